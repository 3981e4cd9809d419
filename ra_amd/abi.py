"""numpy mirrors of the C-ABI structs and constants in include/ra_gpu_batch.h.

Every array that crosses the boundary is a numpy structured array whose dtype below has the
exact C layout (verified against rgb_struct_size() when the library loads).  Field meanings
follow the reference's wire records (reference src/ra.hrl:123-154) -- see the header.
"""
from __future__ import annotations

import numpy as np

ABI_VERSION = 10
ABI_MINOR = 1                  # RGB_ABI_MINOR: 1 = the compact decision forms expand_decisions reads (a superset of minor 0's)
CFG_ROUNDS_PER_LAUNCH = 1      # rgb_config.flags: rgb_submit launches one kernel per sub-tick round (the default since round 5)
CFG_SUBMIT_TRAINS = 16         # rgb_config.flags: opt-in -- rgb_submit fuses the sub-tick rounds of a batch into one train launch
CFG_FUSE_PIPELINE = 4          # rgb_config.flags: a leader's success reply / written event carries its pipeline_rpcs event's rpcs (opt-in)
CFG_TRAIN_PERSISTENT = 2       # rgb_config.flags: trains always in the persistent form (placement by construction)
UNDEF = np.uint64(0xFFFFFFFFFFFFFFFF)  # Erlang 'undefined'
UNDEF_INT = 0xFFFFFFFFFFFFFFFF
NONE = 0xFF                            # undefined member slot
MAX_MEMBERS = 8
MAX_RUNS = 16
AER_CHUNK_SIZE = 128
DEFAULT_MAX_PIPELINE_COUNT = 4096

# ra_state()
ROLE_FOLLOWER, ROLE_CANDIDATE, ROLE_LEADER, ROLE_PRE_VOTE, ROLE_AWAIT_CONDITION = range(5)
ROLE_NAMES = ["follower", "candidate", "leader", "pre_vote", "await_condition"]
(COND_NONE, COND_MISSING, COND_TERM_MISMATCH, COND_WAL_DOWN, COND_WAL_DOWN_LEADER,
 COND_TRANSFER_LEADERSHIP) = range(6)

(MSG_NOP, MSG_AER, MSG_AER_REPLY, MSG_REQUEST_VOTE, MSG_VOTE_RESULT, MSG_WRITTEN,
 MSG_PIPELINE_RPCS, MSG_APPEND, MSG_AWAIT_TIMEOUT, MSG_ELECTION_TIMEOUT, MSG_PRE_VOTE_RPC,
 MSG_PRE_VOTE_RESULT, MSG_SNAPSHOT_WRITTEN, MSG_HEARTBEAT_RPC, MSG_HEARTBEAT_REPLY,
 MSG_CONSISTENT_QUERY, MSG_TRANSFER_LEADERSHIP) = range(17)
N_KINDS = 17
PROTO_VERSION = 1
# device order of a tick: clause family = (class rank of the kind, success flag); the four hot
# kinds first (each has a specialised kernel), the rest after (ra_amd/csrc/rgb_internal.h); the two cold
# leader-side calls (consistent query, transfer_leadership) share rank 14
KIND_RANK = np.array([15, 0, 1, 5, 6, 2, 4, 3, 7, 8, 9, 10, 11, 12, 13, 14, 14], dtype=np.int64)
MF_SUCCESS = 0x01
MF_FORCE = 0x02
MF_TICK = 0x04
MF_SEQ2 = 0x08
MF_CAN_WRITE = 0x10
MF_SEQX = 0x20       # WRITTEN (with MF_SEQ2): more than two ranges, the lower ones in the batch's range list (c, n_entries)

F_REPLY = 1 << 0
F_REPLY_SUCCESS = 1 << 1
F_REPLY_VOTE = 1 << 2
F_PERSIST = 1 << 3
F_LEADER_MSG = 1 << 4
F_LEADER_CHANGED = 1 << 5
F_APPLIED = 1 << 6
F_AUX_EVAL = 1 << 7
F_WROTE = 1 << 8
F_TRUNCATED = 1 << 9
F_PIPELINE = 1 << 10
F_REPROCESSED = 1 << 11
F_ROLE_CHANGED = 1 << 12
F_BECAME_LEADER = 1 << 13
F_UNHANDLED = 1 << 14
F_INVARIANT = 1 << 15
F_RUNS_OVERFLOW = 1 << 16
F_SEND_SNAPSHOT = 1 << 17
F_REPLY_PRE_VOTE = 1 << 18
F_START_ELECTION_TIMEOUT = 1 << 19
F_SEND_VOTE_REQUESTS = 1 << 20
F_PRE_VOTE_REQS = 1 << 21
F_RESEND_PENDING = 1 << 22
F_REPLY_HEARTBEAT = 1 << 23
F_SEND_HEARTBEATS = 1 << 24
F_QUERY_QUORUM = 1 << 25
F_QUERY_APPLY = 1 << 26
F_CANCEL_SNAPSHOT_RETRY = 1 << 27
F_TRANSFER_LEADERSHIP = 1 << 29   # leader's wal_down condition timed out: {transfer_leadership, Peer} (src/ra_server.erl:660-668)
F_COMPACT = 1 << 28   # device-resident decision streams: the 32-byte compact form (expand_decisions)
F_CALL_REPLY = 1 << 30   # {reply, Reply} to a call's caller: CALL_* in reply_next_index, CALL_OK's send_msg target in reply_to

# rgb_decision.reply_next_index under F_CALL_REPLY: handle_leader({transfer_leadership, T}, _) src/ra_server.erl:996-1035
(CALL_OK, CALL_ALREADY_LEADER, CALL_UNKNOWN_MEMBER, CALL_NON_VOTER, CALL_NOT_UP_TO_DATE, CALL_UNSUPPORTED) = range(6)

(INV_NONE, INV_LEADER_SAW_AER_SAME_TERM, INV_TRUNCATE_BELOW_APPLIED, INV_WRITE_BELOW_APPLIED,
 INV_MISMATCH_TERM_UNDEFINED, INV_WRITE_INTEGRITY, INV_SET_LAST_INDEX_NOT_FOUND,
 INV_LAST_WRITTEN_TERM, INV_NEXT_INDEX_REGRESSED, INV_PIPELINE_PREV_UNDEFINED,
 INV_WRITTEN_NOT_PREFIX, INV_LEADER_SAW_HEARTBEAT_SAME_TERM) = range(12)

RPC_AER, RPC_SNAPSHOT = 1, 2

OK, E_INVAL, E_NOMEM, E_HIP, E_STATE, E_FULL, E_EMPTY, E_UNSUPPORTED, E_NODEVICE, E_COMM = (
    0, -1, -2, -3, -4, -5, -6, -7, -8, -9)
COMM_ID_BYTES = 128

u8, u16, u32, u64, i32 = np.uint8, np.uint16, np.uint32, np.uint64, np.int32

MSG_DTYPE = np.dtype([
    ("server", u32), ("kind", u8), ("from", u8), ("flags", u8), ("gap", u8),
    ("term", u64), ("a", u64), ("b", u64), ("c", u64),
    ("n_entries", u32), ("n_run0", u32), ("run0_term", u64), ("run1_term", u64),
])

DECISION_DTYPE = np.dtype([
    ("server", u32), ("role", u8), ("reply_to", u8), ("n_rpcs", u8), ("kind", u8),
    ("flags", u32), ("invariant", u16), ("heartbeat_to", u8), ("cancel_backoff", u8),
    ("reply_term", u64), ("reply_next_index", u64), ("reply_last_index", u64),
    ("reply_last_term", u64), ("commit_index", u64), ("last_applied", u64),
])

RPC_DTYPE = np.dtype([
    ("msg_index", u32), ("server", u32), ("peer", u8), ("kind", u8), ("n_entries", u16),
    ("_pad", u32),
    ("term", u64), ("prev_log_index", u64), ("prev_log_term", u64), ("leader_commit", u64),
    ("next_index", u64),
])

SERVER_STATE_DTYPE = np.dtype([
    ("current_term", u64), ("commit_index", u64), ("last_applied", u64),
    ("last_index", u64), ("last_term", u64),
    ("last_written_index", u64), ("last_written_term", u64),
    ("snapshot_index", u64), ("snapshot_term", u64), ("first_index", u64),
    ("cond_reply", u64, (4,)),
    ("match_index", u64, (MAX_MEMBERS,)), ("next_index", u64, (MAX_MEMBERS,)),
    ("commit_index_sent", u64, (MAX_MEMBERS,)),
    ("run_start", u64, (MAX_RUNS,)), ("run_term", u64, (MAX_RUNS,)),
    ("role", u8), ("cond_reason", u8), ("self", u8), ("n_members", u8),
    ("voted_for", u8), ("leader_id", u8), ("votes", u8), ("n_runs", u8),
    ("present_mask", u8), ("voter_mask", u8), ("status_mask", u8), ("self_nonvoter", u8),
    ("cond_leader", u8), ("backoff_mask", u8), ("n_pending_old", u8), ("_pad", u8, (1,)),
    ("pre_vote_token", u64), ("query_index", u64), ("peer_query_index", u64, (MAX_MEMBERS,)),
    ("pending_first", u64),
    ("machine_version", u32), ("effective_machine_version", u32),
    ("pending_old", u64, (2, 2)),
])

LEADERBOARD_DTYPE = np.dtype([
    ("leader", u32), ("n_leaders", u32), ("term", u64), ("commit_index", u64),
    ("last_applied", u64),
])

CONFIG_DTYPE = np.dtype([
    ("abi_version", u32), ("device", i32), ("max_runs", u32), ("ring_slots", u32),
    ("ring_capacity", u32), ("max_pipeline_count", u32), ("max_aer_batch", u32), ("flags", u32),
])

# include/ra_gpu_wal.h
WAL_ENTRY_DTYPE = np.dtype([("index", u64), ("term", u64), ("data_offset", u64), ("data_len", u32),
                            ("_pad", u32)])
assert WAL_ENTRY_DTYPE.itemsize == 32
WAL_RECORD_DTYPE = np.dtype([("index", u64), ("term", u64), ("data_offset", u64), ("data_len", u32),
                             ("hdr_len", u32), ("hdr_offset", u64), ("out_offset", u64)])
assert WAL_RECORD_DTYPE.itemsize == 48
WAL_SCANNED_DTYPE = np.dtype([("index", u64), ("term", u64), ("data_offset", u64), ("data_len", u32),
                              ("checksum", u32), ("uid_offset", u64), ("id_ref", u32), ("uid_len", np.uint16),
                              ("trunc", np.uint8), ("flags", np.uint8), ("next_offset", u64)])
assert WAL_SCANNED_DTYPE.itemsize == 56
WAL_NO_CHECKSUMS = 1
WAL_REC_FIRST, WAL_REC_VALIDATE, WAL_REC_UNKNOWN = 1, 2, 4
WAL_END_ZEROS, WAL_END_DATA, WAL_END_CAP = 0, 1, 2
WAL_CLEAN, WAL_DROPPED_LAST, WAL_CORRUPT = 0, 1, 2
WAL_FILE_HEADER = b"RAWA\x01"
# WAL batch (same header): a command, a writer slot, the file, a command's result, a written event, the total
WAL_CMD_DTYPE = np.dtype([("writer", u32), ("data_len", u32), ("index", u64), ("term", u64), ("prev_index", u64),
                          ("smallest_index", u64), ("tid", u64), ("data_offset", u64), ("_pad", u64)])
WAL_WRITER_DTYPE = np.dtype([("state", u32), ("id_ref", u32), ("prev_index", u64), ("uid_offset", u64),
                             ("uid_len", u32), ("_pad", u32)])
WAL_FILE_DTYPE = np.dtype([("file_size", u64), ("entry_count", u64), ("max_size", u64), ("max_entries", u64),
                           ("next_id_ref", u32), ("_pad", u32)])
WAL_CMD_RESULT_DTYPE = np.dtype([("verdict", u32), ("checksum", u32), ("value", u64)])
WAL_EVENT_DTYPE = np.dtype([("writer", u32), ("range_first", u32), ("term", u64), ("tid", u64), ("range_n", u32),
                            ("_pad", u32)])
WAL_BATCH_TOTAL_DTYPE = np.dtype([("status", u32), ("n_consumed", u32), ("n_written", u32), ("n_events", u32),
                                  ("n_ranges", u32), ("next_id_ref", u32), ("out_bytes", u64), ("file_size", u64),
                                  ("entry_count", u64), ("_pad", u64, (2,))])
assert (WAL_CMD_DTYPE.itemsize, WAL_WRITER_DTYPE.itemsize, WAL_FILE_DTYPE.itemsize, WAL_CMD_RESULT_DTYPE.itemsize,
        WAL_EVENT_DTYPE.itemsize, WAL_BATCH_TOTAL_DTYPE.itemsize) == (64, 32, 40, 16, 32, 64)
WAL_W_UNDEFINED, WAL_W_IN_SEQ, WAL_W_OUT_OF_SEQ = range(3)
WAL_NO_ID_REF, WAL_MAX_ID_REFS = 0xFFFFFFFF, 1 << 22
WAL_V_NOT_CONSUMED, WAL_V_WRITE, WAL_V_DROP, WAL_V_IGNORE, WAL_V_RESEND = range(5)
WAL_V_MASK, WAL_V_TRUNC, WAL_V_FIRST = 0xFF, 0x100, 0x200
WAL_BATCH_OK, WAL_BATCH_ROLL, WAL_BATCH_SPACE = range(3)
# segments and snapshots (same header)
SEG_ENTRY_DTYPE = np.dtype([("index", u64), ("term", u64), ("data_offset", u64), ("data_len", u32), ("crc", u32)])
assert SEG_ENTRY_DTYPE.itemsize == 32
SEG_NO_CHECKSUMS = 1
SEG_VERSION, SEG_HEADER_BYTES, SEG_RECORD_BYTES, SEG_RECORD_BYTES_V1 = 2, 8, 32, 28
SEG_END_ZEROS, SEG_END_FULL, SEG_END_TRUNCATED, SEG_END_CAP = 0, 1, 2, 3
SEG_MAX_ENTRIES, SEG_MAX_SIZE_B = 4096, 64_000_000            # src/ra.hrl:225, 227
# major compaction (same header): one source file of a group, its info/2 row, the result of the copy
SEG_SOURCE_DTYPE = np.dtype([("offset", u64), ("n_bytes", u64), ("live_first", u32), ("live_n", u32), ("_pad", u64)])
SEG_INFO_DTYPE = np.dtype([("size", u64), ("index_size", u64), ("live_size", u64), ("range_first", u64),
                           ("range_last", u64), ("num_entries", u32), ("num_indexes", u32), ("max_count", u32),
                           ("version", u32), ("status", u32), ("_pad", u32)])
SEG_COMPACT_RESULT_DTYPE = np.dtype([("status", u32), ("n_entries", u32), ("file_bytes", u64), ("index", u64),
                                     ("source", u32), ("_pad", u32)])
assert (SEG_SOURCE_DTYPE.itemsize, SEG_INFO_DTYPE.itemsize, SEG_COMPACT_RESULT_DTYPE.itemsize) == (32, 64, 32)
(SEG_COMPACT_OK, SEG_COMPACT_MISSING, SEG_COMPACT_FULL, SEG_COMPACT_TRUNCATED, SEG_COMPACT_SPACE, SEG_COMPACT_CRC,
 SEG_COMPACT_BAD_SOURCE) = range(7)
SEG_COMPACT_VERIFY = 1
SEG_COMPACT_MAX_SOURCES = 256
# major compaction for many members (same header): the plan's descriptors and a group of the batched copy
SEG_MEMBER_DTYPE = np.dtype([("segref_first", u32), ("segref_n", u32), ("live_first", u32), ("live_n", u32)])
SEG_PICK_DTYPE = np.dtype([("num_live", u64), ("live_first", u32), ("live_n", u32), ("flags", u32), ("_pad", u32)])
SEG_TAKE_MEMBER_DTYPE = np.dtype([("src_first", u32), ("src_n", u32), ("n_groups", u32), ("status", u32)])
SEG_GROUP_DTYPE = np.dtype([("src_first", u32), ("src_n", u32), ("out_offset", u64), ("out_bytes", u64)])
assert (SEG_MEMBER_DTYPE.itemsize, SEG_PICK_DTYPE.itemsize, SEG_TAKE_MEMBER_DTYPE.itemsize,
        SEG_GROUP_DTYPE.itemsize) == (16, 24, 16, 24)
SEG_PICK_UNREFERENCED = 1
SEG_TAKE_OK, SEG_TAKE_BADARITH = 0, 1
SEG_GROUP_NONE = 0xFFFFFFFF
# mem-table flush (same header): one writer of a call, one run of appended entries in one file, the result
SEG_WRITER_DTYPE = np.dtype([("entry_first", u32), ("entry_n", u32), ("open_count", u32), ("open_max_count", u32),
                             ("open_data_bytes", u64), ("range_first", u64), ("range_last", u64), ("_pad", u64)])
SEG_PIECE_DTYPE = np.dtype([("writer", u32), ("ordinal", u32), ("entry_first", u32), ("entry_n", u32),
                            ("index_file_off", u64), ("data_file_off", u64), ("out_index_off", u64),
                            ("out_data_off", u64), ("data_bytes", u64), ("range_first", u64), ("range_last", u64),
                            ("max_count", u32), ("_pad", u32)])
SEG_FLUSH_RESULT_DTYPE = np.dtype([("status", u32), ("n_pieces", u32), ("out_bytes", u64), ("writer", u32),
                                   ("entry", u32), ("_pad", u64)])
assert (SEG_WRITER_DTYPE.itemsize, SEG_PIECE_DTYPE.itemsize, SEG_FLUSH_RESULT_DTYPE.itemsize) == (48, 80, 32)
SEG_FLUSH_OK, SEG_FLUSH_SPACE, SEG_FLUSH_ENTRY = range(3)
# reading entries back (same header): one source of a call, its result, the call's total; the rows are SEG_ENTRY_DTYPE
SEG_READ_SOURCE_DTYPE = np.dtype([("offset", u64), ("n_bytes", u64), ("req_first", u32), ("req_n", u32), ("_pad", u64)])
SEG_READ_RESULT_DTYPE = np.dtype([("status", u32), ("n_read", u32), ("index", u64), ("data_bytes", u64), ("_pad", u64)])
SEG_READ_TOTAL_DTYPE = np.dtype([("status", u32), ("n_bad", u32), ("out_bytes", u64)])
assert (SEG_READ_SOURCE_DTYPE.itemsize, SEG_READ_RESULT_DTYPE.itemsize, SEG_READ_TOTAL_DTYPE.itemsize) == (32, 32, 16)
(SEG_READ_OK, SEG_READ_MISSING, SEG_READ_TRUNCATED, SEG_READ_CRC, SEG_READ_BAD_SOURCE, SEG_READ_SPACE) = range(6)
SEG_READ_VERIFY, SEG_READ_NO_DATA = 1, 2
SEG_READ_MAX_SOURCES = 65536
# snapshots and checkpoints (same header): a span of a ragged CRC batch, an image to write, a file to check, its row
CRC_SPAN_DTYPE = np.dtype([("offset", u64), ("n_bytes", u64), ("init", u32), ("_pad", u32), ("_pad2", u64)])
SNAP_ITEM_DTYPE = np.dtype([("kind", u32), ("meta_len", u32), ("meta_offset", u64), ("data_offset", u64),
                            ("data_bytes", u64), ("out_offset", u64)])
SNAP_FILE_DTYPE = np.dtype([("offset", u64), ("n_bytes", u64), ("kind", u32), ("flags", u32), ("_pad", u64)])
SNAP_INFO_DTYPE = np.dtype([("status", u32), ("version", u32), ("stored_crc", u32), ("computed_crc", u32),
                            ("meta_offset", u64), ("meta_len", u32), ("_pad", u32), ("data_offset", u64),
                            ("data_bytes", u64)])
assert (CRC_SPAN_DTYPE.itemsize, SNAP_ITEM_DTYPE.itemsize, SNAP_FILE_DTYPE.itemsize, SNAP_INFO_DTYPE.itemsize) == \
    (32, 40, 32, 48)
SNAP_KIND_SNAPSHOT, SNAP_KIND_INDEXES = 0, 1
SNAP_HEADER_BYTES, SNAP_META_HEADER_BYTES = 9, 13
SNAP_META_ONLY = 1
(SNAP_OK, SNAP_INVALID_FORMAT, SNAP_INVALID_VERSION, SNAP_CHECKSUM, SNAP_BAD_META, SNAP_EOF) = range(6)

# rgb_view (ABI v9, rgb_collect_view): pointers into the pinned slot the device wrote
VIEW_DTYPE = np.dtype([("decisions", "<u8"), ("rpcs", "<u8"), ("tick", "<u8"), ("n", "<u4"), ("n_rpcs", "<u4"),
                       ("slot", "<u4"), ("_pad", "<u4")])
# rgb_fill (rgb_submit_begin): the slot's pinned message buffer, handed to the producer
FILL_DTYPE = np.dtype([("msgs", "<u8"), ("cap", "<u4"), ("slot", "<u4"), ("max_rounds", "<u4"), ("_pad", "<u4")])
SUBMIT_RAW_MAX_ROUNDS = 8
STRUCT_DTYPES = [MSG_DTYPE, DECISION_DTYPE, RPC_DTYPE, SERVER_STATE_DTYPE, LEADERBOARD_DTYPE,
                 CONFIG_DTYPE, VIEW_DTYPE, FILL_DTYPE]
EXPECTED_SIZES = [64, 64, 56, 704, 32, 32, 40, 24]
for _dt, _sz in zip(STRUCT_DTYPES, EXPECTED_SIZES):
    assert _dt.itemsize == _sz, (_dt, _dt.itemsize, _sz)


def family(msgs: np.ndarray) -> np.ndarray:
    return KIND_RANK[msgs["kind"]] * 2 + (msgs["flags"] & MF_SUCCESS)


def empty_server_states(n_groups: int, n_members: int) -> np.ndarray:
    """ra_server:init/1 on an empty log for every member of every group: the `empty_state/2`
    fixture of the reference's tests (test/ra_server_SUITE.erl:4139-4149): term 0, log [0:0]
    written, every peer new_peer/0 (src/ra_server.erl:2990-2995)."""
    n = n_groups * n_members
    st = np.zeros(n, dtype=SERVER_STATE_DTYPE)
    st["snapshot_index"] = UNDEF
    st["snapshot_term"] = UNDEF
    st["next_index"][:, :n_members] = 1   # slots beyond n_members stay 0 (canonical form)
    st["pending_first"] = 1               # nothing pending: last_index + 1
    st["role"] = ROLE_FOLLOWER
    st["self"] = np.arange(n, dtype=np.uint32) % n_members
    st["n_members"] = n_members
    st["voted_for"] = NONE
    st["leader_id"] = NONE
    st["cond_leader"] = NONE
    st["n_runs"] = 1  # run 0 = (start 0, term 0)
    st["present_mask"] = (1 << n_members) - 1
    st["voter_mask"] = (1 << n_members) - 1
    st["status_mask"] = 0xFF
    return st


def set_log(st: np.ndarray, i: int, entries, last_written=None, snapshot=None, first_index=None):
    """Fill server i's log cursors from an explicit [(index, term), ...] list (ascending,
    contiguous), the notation of the reference's tests: `[{1,1},{2,3},{3,5}]`."""
    s = st[i:i + 1]
    if snapshot is not None:
        s["snapshot_index"], s["snapshot_term"] = snapshot
    entries = list(entries)
    if entries:
        fi = entries[0][0] if first_index is None else first_index
        s["first_index"] = fi
        s["last_index"], s["last_term"] = entries[-1]
        runs = []
        prev = None
        for k, (idx, term) in enumerate(entries):
            assert idx == entries[0][0] + k, "log entries must be contiguous"
            if prev is None or term != prev:
                runs.append((idx, term))
                prev = term
        assert len(runs) <= MAX_RUNS
        s["n_runs"] = len(runs)
        s["run_start"] = 0
        s["run_term"] = 0
        for r, (a, t) in enumerate(runs):
            st["run_start"][i, r] = a
            st["run_term"][i, r] = t
    else:
        assert snapshot is not None, "an empty range needs a snapshot"
        s["last_index"], s["last_term"] = snapshot
        s["first_index"] = snapshot[0] + 1
        s["n_runs"] = 0
    if last_written is None:
        last_written = (int(s["last_index"][0]), int(s["last_term"][0]))
    s["last_written_index"], s["last_written_term"] = last_written
    # ra_log `pending`: the unwritten tail is what the WAL still owes (empty = last_index + 1)
    s["pending_first"] = min(int(last_written[0]), int(s["last_index"][0])) + 1


def log_entries(st_row) -> list:
    """Inverse of set_log for one state row: [(index, term), ...] of the ra_log range."""
    out = []
    fi, li = int(st_row["first_index"]), int(st_row["last_index"])
    if fi > li:
        return out
    nr = int(st_row["n_runs"])
    for r in range(nr):
        a = int(st_row["run_start"][r])
        b = int(st_row["run_start"][r + 1]) - 1 if r + 1 < nr else li
        t = int(st_row["run_term"][r])
        out.extend((i, t) for i in range(a, b + 1))
    return out


F_COMPACT_PLAIN = F_LEADER_MSG | F_APPLIED | F_AUX_EVAL | F_PIPELINE      # flags that carry no words of their own
F_COMPACT_CHANGE = F_PERSIST | F_LEADER_CHANGED | F_REPROCESSED | F_ROLE_CHANGED     # .. nor do the flags of a change
COMPACT_FORM_NAMES = ("full", "counted", "wrote", "confirmed", "answered", "stood")
_COUNTED_KINDS = (MSG_AER_REPLY, MSG_WRITTEN, MSG_AER, MSG_VOTE_RESULT, MSG_APPEND, MSG_PRE_VOTE_RESULT,
                  MSG_SNAPSHOT_WRITTEN, MSG_HEARTBEAT_RPC)


def compact_forms(dec: np.ndarray) -> np.ndarray:
    """Which compact form (index into COMPACT_FORM_NAMES, 0 = none) the encoder of include/ra_gpu_batch.h gives each
    FULL record of `dec`: the classification of compact_decision (rgb_kernels.hip) on the host, for counting and tests."""
    d = np.asarray(dec, dtype=DECISION_DTYPE)
    u = np.uint64
    kind, flags = d["kind"], d["flags"]
    shape = flags & ~np.uint32(F_COMPACT_PLAIN)
    stem = shape & ~np.uint32(F_COMPACT_CHANGE)
    term, nxt, last, lterm, ci, la = (d[f] for f in ("reply_term", "reply_next_index", "reply_last_index",
                                                    "reply_last_term", "commit_index", "last_applied"))
    ok = (d["invariant"] == 0) & (d["heartbeat_to"] == 0) & (d["cancel_backoff"] == 0) & ((flags & F_COMPACT) == 0)
    form = np.zeros(len(d), dtype=np.uint8)
    with np.errstate(over="ignore"):
        def within(hi, lo, limit):          # 0 <= hi - lo <= limit in the integers
            return (hi >= lo) & (hi - lo <= u(limit))

        def biased(hi, lo, bias, limit):    # 0 <= hi + bias - lo <= limit in the integers
            up = hi >= lo
            return np.where(up, hi - lo, lo - hi) <= np.where(up, u(limit - bias), u(bias))

        aer = (kind == MSG_AER) & ((stem == shape) | ((shape & (F_ROLE_CHANGED | F_LEADER_CHANGED)) != 0))
        counted = (((shape == 0) & np.isin(kind, _COUNTED_KINDS)) |
                   ((kind == MSG_VOTE_RESULT) & (shape == (F_BECAME_LEADER | F_ROLE_CHANGED | F_LEADER_CHANGED)))) & \
            ((term | nxt | last | lterm) == 0)
        counted |= (kind == MSG_HEARTBEAT_REPLY) & (shape == F_QUERY_QUORUM) & ((term | last | lterm) == 0) & \
            (nxt <= u(0xFFFFFFFF))
        wrote = (stem == F_WROTE) & aer & ((term | lterm) == 0) & within(last, nxt, 0xFFFF) & within(last, la, 0xFFFF)
        A = nxt - u(1)
        confirmed = (stem == (F_REPLY | F_REPLY_SUCCESS)) & (aer | ((kind == MSG_WRITTEN) & (stem == shape))) & (nxt != 0) & \
            within(A, last, 0xFF) & within(term, lterm, 0xF) & biased(ci, A, 512, 0x3FF) & within(nxt, la, 0x3FF)
        answered = (kind == MSG_HEARTBEAT_RPC) & (stem == (F_REPLY | F_REPLY_HEARTBEAT)) & ((last | lterm) == 0) & \
            (nxt <= u(0xFFFF)) & biased(ci, la, 0x8000, 0xFFFF)
        stood = (kind == MSG_PRE_VOTE_RESULT) & (stem == F_SEND_VOTE_REQUESTS) & (nxt == 0) & within(term, lterm, 0xFF) & \
            within(last, ci, 0xFFF) & within(last, la, 0xFFF)
    for k, m in enumerate((counted, wrote, confirmed, answered, stood), 1):
        form[ok & m] = k
    return form


def expand_decisions(dec: np.ndarray) -> np.ndarray:
    """rgb_decision_expand (include/ra_gpu_batch.h) over an array read from a DEVICE-RESIDENT decision stream: records
    with F_COMPACT were written as 32 bytes; the full records come back (a copy), the flag cleared."""
    d = np.array(dec, dtype=DECISION_DTYPE, copy=True)
    c = (d["flags"] & F_COMPACT) != 0
    if not c.any():
        return d
    w = d.view(np.uint64).reshape(-1, 8)
    aux = (w[:, 1] >> np.uint64(32)).astype(np.uint64)
    A, B = w[:, 2].copy(), w[:, 3].copy()
    flags = d["flags"] & ~np.uint32(F_COMPACT)
    rest = c.copy()

    def take(mask):
        m = rest & mask
        rest[m] = False
        return m

    answered = take((flags & F_REPLY_HEARTBEAT) != 0)
    confirmed = take((flags & F_REPLY) != 0)
    wrote = take((flags & F_WROTE) != 0)
    stood = take((flags & F_SEND_VOTE_REQUESTS) != 0)
    counted = rest
    with np.errstate(over="ignore"):
        d["flags"] = flags
        for f in ("invariant", "heartbeat_to", "cancel_backoff"):
            d[f][c] = 0
        for f in ("reply_term", "reply_next_index", "reply_last_index", "reply_last_term"):
            d[f][c] = 0
        u = np.uint64

        def put(m, **fields):
            for f, v in fields.items():
                d[f][m] = v[m]

        put(answered, commit_index=A, reply_term=B, reply_next_index=aux & u(0xFFFF),
            last_applied=A + u(32768) - (aux >> u(16)))
        put(confirmed, reply_next_index=A + u(1), reply_term=B, reply_last_index=A - (aux & u(0xFF)),
            reply_last_term=B - ((aux >> u(8)) & u(0xF)), commit_index=A + ((aux >> u(12)) & u(0x3FF)) - u(512),
            last_applied=A + u(1) - ((aux >> u(22)) & u(0x3FF)))
        put(wrote, reply_last_index=A, reply_next_index=A - (aux & u(0xFFFF)), commit_index=B,
            last_applied=A - (aux >> u(16)))
        put(stood, reply_last_index=A, reply_term=B, reply_last_term=B - (aux & u(0xFF)),
            commit_index=A - ((aux >> u(8)) & u(0xFFF)), last_applied=A - (aux >> u(20)))
        put(counted, commit_index=A, last_applied=B, reply_next_index=aux)
    return d
