"""One-call WAL batch: rgb_wal_batch_bound / rgb_wal_batch_device / rgb_wal_batch (include/ra_gpu_wal.h, "WAL batch";
ra_amd/csrc/rgb_wal.hip, rgb_wal_host.cpp).

Referee: `referee` below is the literal loop of ra_log_wal:handle_batch/2 over append commands, written from the
reference source -- handle_msg/2 (src/ra_log_wal.erl:551-586), write_data/8 with should_roll_wal/1 and
serialize_header/3 (:482-548, :1050-1066), incr_batch/8 (:596-635) and complete_batch_writer/3 (:800-812) -- one command
after the other, the ra_seq of a batch writer kept with tests/ra_log_model.py's seq_append / seq_limit / seq_floor.  The
library decides per writer, scans in mailbox order and keeps a run's indexes as a stack of pairs; the referee
deliberately does none of that.

Every device check exists twice: on the CPU emulation of the same sources (-m "not gpu") and on the GPU."""
import json
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from emu_schedule import PERMUTED_SCHEDULES, schedule
from ra_amd import abi
from ra_amd.engine import RgbError
from ra_log_model import seq_append, seq_expand, seq_floor, seq_limit
from test_segment import Emu, Gpu, emu, gpu, first_diff                                  # noqa: F401  (fixtures)
from test_wal_framing import (SWEEP_LARGE, SWEEP_MID, SWEEP_SMALL, header_bytes, phase_sweep_batch, python_frame)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL = -1
TILE = 256                     # rgb_wal.hip: commands per workgroup step of the scan (WB_THREADS)
CHUNK = 64                     # ... and commands of a writer per LDS chunk at the widest sub-group
UNDEFINED, IN_SEQ, OUT_OF_SEQ = abi.WAL_W_UNDEFINED, abi.WAL_W_IN_SEQ, abi.WAL_W_OUT_OF_SEQ
WRITE, DROP, IGNORE, RESEND, NOT_CONSUMED = (abi.WAL_V_WRITE, abi.WAL_V_DROP, abi.WAL_V_IGNORE, abi.WAL_V_RESEND,
                                             abi.WAL_V_NOT_CONSUMED)
OK, ROLL, SPACE = abi.WAL_BATCH_OK, abi.WAL_BATCH_ROLL, abi.WAL_BATCH_SPACE
BIG = 1 << 40                  # a max_size nothing here reaches


# ------------------------------------------------------------------------------------------ referee

class Cmd:
    def __init__(self, writer, idx, term, prev, smallest, tid, payload):
        self.writer, self.idx, self.term, self.prev, self.smallest, self.tid, self.payload = \
            writer, idx, term, prev, smallest, tid, payload


class Writer:
    """state: None | ("in_seq", P) | ("out_of_seq", P); id_ref: the writer-name cache's entry for this file or None"""

    def __init__(self, uid, state=None, id_ref=None):
        self.uid, self.state, self.id_ref = uid, state, id_ref


def referee(cmds, writers, file_size, entry_count, next_id_ref, max_size, max_entries, checksums=True):
    """-> dict(rows=[(verdict, trunc, first, value)], specs (for python_frame), payloads, out, writers=[(state, id_ref)],
    events=[(writer, term, tid, frozenset)], status, n_consumed, n_written, file_size, entry_count, next_id_ref)"""
    state = {w: wr.state for w, wr in enumerate(writers)}
    cache = {w: wr.id_ref for w, wr in enumerate(writers) if wr.id_ref is not None}
    waiting = {}                                      # writer -> [batch_writer, oldest first] (the `old` chain)
    rows, specs, payloads, pending = [], [], [], []
    status, n_consumed, real = OK, len(cmds), 0
    for pos, c in enumerate(cmds):
        trunc = c.idx == c.smallest
        st = state[c.writer]
        if c.idx < c.smallest:
            state[c.writer] = ("in_seq", c.smallest - 1)
            rows.append((DROP, 0, 0, 0))
            continue
        if st is not None and (c.prev <= st[1] or trunc):
            pass
        elif st is None:
            trunc = False
        elif st[0] == "out_of_seq":
            rows.append((IGNORE, 0, 0, 0))
            continue
        else:
            rows.append((RESEND, 0, 0, st[1] + 1))
            state[c.writer] = ("out_of_seq", st[1])
            continue
        # write_data/8
        if file_size > max_size or (max_entries and entry_count + 1 > max_entries):
            status, n_consumed = ROLL, pos
            break
        if c.writer in cache:
            spec_uid, id_ref = None, cache[c.writer]
            header_len = 2 if trunc else 3
        else:
            spec_uid, id_ref = writers[c.writer].uid, next_id_ref
            cache[c.writer] = next_id_ref
            next_id_ref += 1
            header_len = 5 + len(spec_uid)
        specs.append((int(trunc), id_ref, spec_uid, c.idx, c.term, len(c.payload)))
        payloads.append(c.payload)
        entry = struct.pack(">QQ", c.idx, c.term) + c.payload
        cs = zlib.adler32(entry) if checksums else 0
        record = header_bytes(int(trunc), id_ref, spec_uid) + struct.pack(">II", cs, len(c.payload)) + entry
        rows.append((WRITE, int(trunc), int(spec_uid is not None), real, cs))
        pending.append(record)
        real += len(record)
        # incr_batch/8
        chain = waiting.setdefault(c.writer, [])
        if chain and chain[-1]["term"] == c.term and chain[-1]["tid"] == c.tid:
            bw = chain[-1]
            bw["seq"] = seq_append(c.idx, seq_limit(c.idx - 1, bw["seq"]))
            bw["smallest"] = c.smallest
        else:
            chain.append(dict(term=c.term, tid=c.tid, seq=seq_append(c.idx, []), smallest=c.smallest))
        file_size += header_len + 24 + len(c.payload)
        entry_count += 1
        state[c.writer] = ("in_seq", c.idx)
    rows += [(NOT_CONSUMED, 0, 0, 0)] * (len(cmds) - len(rows))
    events = []
    for w in sorted(waiting):                         # complete_batch_writer/3: the old ones first
        for bw in waiting[w]:
            idxs = seq_expand(seq_floor(bw["smallest"], bw["seq"]))
            assert idxs, "an event without an index"
            events.append((w, bw["term"], bw["tid"], frozenset(idxs)))
    return dict(rows=rows, specs=specs, payloads=payloads, out=b"".join(pending),
                writers=[(state[w], cache.get(w)) for w in range(len(writers))], events=events, status=status,
                n_consumed=n_consumed, n_written=len(specs), file_size=file_size, entry_count=entry_count,
                next_id_ref=next_id_ref)


# ------------------------------------------------------------------------------------------ building inputs

def pack(rng, cmds, writers, file_size=0, entry_count=0, next_id_ref=0, max_size=BIG, max_entries=0):
    """-> (cmds, writers, file, data) as the arrays of the ABI; payloads and uids at arbitrary alignment in `data`"""
    chunks, pos = [], 0

    def put(b):
        nonlocal pos
        pad = int(rng.integers(0, 7))
        chunks.append(bytes(pad) + b)
        pos += pad + len(b)
        return pos - len(b)

    wa = np.zeros(len(writers), dtype=abi.WAL_WRITER_DTYPE)
    for w, wr in enumerate(writers):
        wa["state"][w] = UNDEFINED if wr.state is None else (IN_SEQ if wr.state[0] == "in_seq" else OUT_OF_SEQ)
        wa["prev_index"][w] = 0 if wr.state is None else wr.state[1]
        wa["id_ref"][w] = abi.WAL_NO_ID_REF if wr.id_ref is None else wr.id_ref
        wa["uid_offset"][w], wa["uid_len"][w] = put(wr.uid), len(wr.uid)
    ca = np.zeros(len(cmds), dtype=abi.WAL_CMD_DTYPE)
    for i, c in enumerate(cmds):
        ca["writer"][i], ca["index"][i], ca["term"][i], ca["prev_index"][i] = c.writer, c.idx, c.term, c.prev
        ca["smallest_index"][i], ca["tid"][i] = c.smallest, c.tid
        ca["data_offset"][i], ca["data_len"][i] = put(c.payload), len(c.payload)
    fa = np.zeros(1, dtype=abi.WAL_FILE_DTYPE)
    fa["file_size"], fa["entry_count"], fa["next_id_ref"] = file_size, entry_count, next_id_ref
    fa["max_size"], fa["max_entries"] = max_size, max_entries
    data = np.frombuffer(b"".join(chunks) + bytes(16), dtype=np.uint8).copy()
    return ca, wa, fa, data


BASES = [1, (1 << 32) - 3, (1 << 63) - 3]


def gen_batch(rng, n, n_writers, lens=(0, 1, 5, 16, 17, 40, 300)):
    """A mailbox of n commands from n_writers clients that misbehave in every way the WAL answers: gaps (a resend
    request, then ignored commands), the resend answered, overwrites with a new tid, term changes inside a run, a
    smallest index that rises mid-batch (drops, then an implicit truncate), Idx == SmallestIdx on writers the WAL knows
    and on ones it does not, uids of 1 and 200 bytes, indexes and terms across 2^32 and 2^63."""
    writers, sh = [], []
    used_refs = int(rng.integers(0, 5))
    for w in range(n_writers):
        uid = bytes(rng.integers(97, 123, size=[1, 200, int(rng.integers(2, 30))][w % 3], dtype=np.uint8))
        base = BASES[int(rng.integers(0, 3))] + int(rng.integers(0, 50))
        kind = int(rng.integers(0, 3))
        state = None if kind == 0 else ("in_seq", base - 1) if kind == 1 else ("out_of_seq", base - 1)
        id_ref = None
        if rng.random() < 0.5:
            id_ref, used_refs = used_refs, used_refs + 1
        writers.append(Writer(uid, state, id_ref))
        small = base if rng.random() < 0.3 else 0                     # Idx == SmallestIdx on the first command
        sh.append(dict(next=base, small=small, term=BASES[int(rng.integers(0, 3))], tid=int(rng.integers(1, 1 << 40)),
                       ahead=0))
    cmds = []
    for _ in range(n):
        w = int(rng.integers(0, n_writers))
        s = sh[w]
        payload = bytes(rng.integers(0, 256, size=int(lens[int(rng.integers(0, len(lens)))]), dtype=np.uint8))
        r = rng.random()
        if s["ahead"]:
            idx = s["next"] + 9 - s["ahead"]
            s["ahead"] -= 1
            cmds.append(Cmd(w, idx, s["term"], idx - 1, s["small"], s["tid"], payload))
            continue
        if r < 0.07:
            s["ahead"] = int(rng.integers(1, 4))                      # a gap, and what the client sends behind it
            continue
        if r < 0.14 and s["next"] > 3:
            s["next"] -= int(rng.integers(1, 4))                      # an overwrite comes with a new mem table
            s["tid"] += 1
            s["term"] += int(rng.integers(0, 2))
        elif r < 0.20:
            s["term"] += 1
        elif r < 0.30:
            s["small"] = max(s["small"], s["next"] + int(rng.integers(-2, 4)))
        idx = s["next"]
        s["next"] += 1
        cmds.append(Cmd(w, idx, s["term"], idx - 1, s["small"], s["tid"], payload))
    while len(cmds) < n:                                              # (a gap draws no command of its own)
        w = int(rng.integers(0, n_writers))
        s = sh[w]
        cmds.append(Cmd(w, s["next"], s["term"], s["next"] - 1, s["small"], s["tid"], b"x"))
        s["next"] += 1
    return cmds[:n], writers, used_refs


# ------------------------------------------------------------------------------------------ comparing

def events_of(events, ranges):
    """-> [(writer, term, tid, frozenset)]; asserts the pairs' form: ascending, not adjacent, first <= last"""
    out = []
    for e in events:
        rf, rn = int(e["range_first"]), int(e["range_n"])
        assert rn >= 1
        idxs, prev_last = [], None
        for f, l in ranges[rf:rf + rn]:
            f, l = int(f), int(l)
            assert f <= l and (prev_last is None or f > prev_last + 1), "pairs not ascending / adjacent"
            assert l - f < 1 << 20
            idxs.extend(range(f, l + 1))
            prev_last = l
        out.append((int(e["writer"]), int(e["term"]), int(e["tid"]), frozenset(idxs)))
    return out


def check_against(ref, got, n_writers, checksums=True):
    total, results, writers_out, out, events, ranges = got
    assert int(total["status"]) == ref["status"]
    for f in ("n_consumed", "n_written", "file_size", "entry_count", "next_id_ref"):
        assert int(total[f]) == ref[f], f
    assert int(total["out_bytes"]) == len(ref["out"])
    for i, row in enumerate(ref["rows"]):
        v = int(results["verdict"][i])
        want_flags = (abi.WAL_V_TRUNC if row[1] else 0) | (abi.WAL_V_FIRST if row[2] else 0)
        assert (v & abi.WAL_V_MASK, v & ~abi.WAL_V_MASK) == (row[0], want_flags), (i, v, row)
        assert int(results["value"][i]) == row[3], (i, row)
        assert int(results["checksum"][i]) == (row[4] if row[0] == WRITE and checksums else 0), (i, row)
    assert ref["out"] == python_frame(ref["specs"], ref["payloads"], checksums)
    d = first_diff(out.tobytes(), ref["out"])
    assert d is None, d
    for w in range(n_writers):
        st, id_ref = ref["writers"][w]
        kind = UNDEFINED if st is None else IN_SEQ if st[0] == "in_seq" else OUT_OF_SEQ
        assert int(writers_out["state"][w]) == kind, w
        if st is not None:
            assert int(writers_out["prev_index"][w]) == st[1], w
        assert int(writers_out["id_ref"][w]) == (abi.WAL_NO_ID_REF if id_ref is None else id_ref), w
    assert int(total["n_events"]) == len(ref["events"]) == len(events)
    assert int(total["n_ranges"]) == len(ranges)
    assert events_of(events, ranges) == ref["events"]
    assert sorted(int(e["range_first"]) for e in events) == [int(e["range_first"]) for e in events]


def run_case(be, rng, cmds, writers, checksums=True, **file):
    ca, wa, fa, data = pack(rng, cmds, writers, **file)
    ref = referee(cmds, writers, int(fa["file_size"][0]), int(fa["entry_count"][0]), int(fa["next_id_ref"][0]),
                  int(fa["max_size"][0]), int(fa["max_entries"][0]), checksums)
    got = be.eng.wal_batch(ca, wa, fa, data, flags=0 if checksums else abi.WAL_NO_CHECKSUMS)
    check_against(ref, got, len(writers), checksums)
    return ref, got


# (n, writers, seed): n around the scan's tile; one writer with every command (a chain of many LDS chunks), one writer
# per command, and a handful
FUZZ_SHAPES = [(1, 1, 11), (TILE - 1, 1, 12), (TILE, TILE, 13), (TILE + 1, 7, 14), (2 * TILE + 3, 1, 15),
               (2 * TILE + 3, 2 * TILE + 3, 16), (2 * TILE + 3, 19, 17), (TILE - 1, 40, 18)]


def fuzz_case(seed, n, n_writers):
    rng = np.random.default_rng(seed)
    cmds, writers, used = gen_batch(rng, n, n_writers)
    return rng, cmds, writers, used


def test_the_generator_reaches_every_clause():
    """A condition, not a hope: over the fuzz shapes the referee alone shows each of the five verdicts, a Trunc header on
    a known writer, Trunc refused on an unknown one, a long header with Trunc, and events cut by the floor."""
    seen = set()
    for n, nw, seed in FUZZ_SHAPES:
        rng, cmds, writers, used = fuzz_case(seed, n, nw)
        # half the shapes roll somewhere inside
        ref = referee(cmds, writers, 0, 0, used, BIG, n // 2 if seed % 2 else 0)
        for row in ref["rows"]:
            seen.add(row[0])
            if row[0] == WRITE and row[1]:
                seen.add("trunc-known" if not row[2] else "trunc-first")
        st = {w: wr.state for w, wr in enumerate(writers)}
        for c in cmds[:ref["n_consumed"]]:
            if st[c.writer] is None and c.idx == c.smallest:
                seen.add("trunc-on-undefined")
            st[c.writer] = 1
        written = {}
        for c, row in zip(cmds, ref["rows"]):
            if row[0] == WRITE:
                written.setdefault(c.writer, set()).add(c.idx)
        if sum(len(e[3]) for e in ref["events"]) < sum(len(v) for v in written.values()):
            seen.add("events-cut")
        if len(ref["events"]) > len(written):
            seen.add("two-runs")
        if ref["status"] == ROLL:
            seen.add("roll")
    assert seen >= {WRITE, DROP, IGNORE, RESEND, NOT_CONSUMED, "trunc-known", "trunc-first", "trunc-on-undefined",
                    "events-cut", "two-runs", "roll"}, seen


def check_fuzz(be, n, n_writers, seed):
    rng, cmds, writers, used = fuzz_case(seed, n, n_writers)
    run_case(be, rng, cmds, writers, next_id_ref=used, max_entries=n // 2 if seed % 2 else 0)


@pytest.mark.parametrize("n,n_writers,seed", FUZZ_SHAPES)
def test_emu_referee_parity(emu, n, n_writers, seed):
    check_fuzz(emu, n, n_writers, seed)


@pytest.mark.parametrize("sched", PERMUTED_SCHEDULES)
def test_emu_referee_parity_under_permuted_schedules(emu, sched):
    for n, n_writers, seed in [(TILE + 1, 7, 14), (2 * TILE + 3, 1, 15), (2 * TILE + 3, 19, 17)]:
        with schedule(emu.engine, sched):
            check_fuzz(emu, n, n_writers, seed)


# ------------------------------------------------------------------------------------------ the reference's suite

def golden_cases():
    with open(os.path.join(ROOT, "tests", "golden", "ra_log_wal_suite_batches.json")) as f:
        doc = json.load(f)
    return doc["uid"].encode(), doc["cases"]


VERDICT_NAMES = {"write": WRITE, "drop": DROP, "ignore": IGNORE, "resend": RESEND, "not_consumed": NOT_CONSUMED}


def golden_inputs(uid, case):
    kind, p = case["writer_state"]
    # a writer the WAL has seen before is in its writer-name cache (the suite's earlier writes went to this file)
    wr = Writer(uid, None if kind == "undefined" else (kind, p), None if kind == "undefined" else 0)
    payload = bytes(range(256)) * (case["payload_len"] // 256 + 1)
    cmds = [Cmd(0, c[0], c[1], c[2], c[3], c[4], payload[:case["payload_len"]]) for c in case["cmds"]]
    return cmds, [wr]


def check_golden(be, case_name):
    uid, cases = golden_cases()
    case = next(c for c in cases if c["name"] == case_name)
    cmds, writers = golden_inputs(uid, case)
    rng = np.random.default_rng(5)
    ref, got = run_case(be, rng, cmds, writers, next_id_ref=1, max_size=case["max_size"], max_entries=case["max_entries"])
    total, results, writers_out, out, events, ranges = got
    assert [int(v) & abi.WAL_V_MASK for v in results["verdict"]] == [VERDICT_NAMES[v] for v in case["verdicts"]]
    assert {str(i): int(results["value"][i]) for i in range(len(cmds))
            if int(results["verdict"][i]) & abi.WAL_V_MASK == RESEND} == case["resend"]
    assert [i for i in range(len(cmds)) if int(results["verdict"][i]) & abi.WAL_V_TRUNC] == case["trunc"]
    assert [(t, tid, sorted(s)) for _, t, tid, s in events_of(events, ranges)] == [tuple(e) for e in case["events"]]
    assert int(total["status"]) == {"ok": OK, "roll": ROLL}[case["status"]]
    assert int(total["n_consumed"]) == case["n_consumed"]
    kind, p = case["writer_after"]
    assert (int(writers_out["state"][0]), int(writers_out["prev_index"][0])) == (IN_SEQ if kind == "in_seq" else OUT_OF_SEQ, p)


GOLDEN_NAMES = [c["name"] for c in golden_cases()[1]]


@pytest.mark.parametrize("case_name", GOLDEN_NAMES)
def test_emu_reference_suite_outcomes(emu, case_name):
    check_golden(emu, case_name)


# ------------------------------------------------------------------------------------------ the accounting quirk

def quirk_case():
    """40 known writers, every record a Trunc record: 26 accounted bytes for 27 written.  max_size is chosen so that the
    roll test by REAL bytes would already be true in front of command k, by accounted bytes only in front of k + 1."""
    n, k = 60, 41
    writers = [Writer(b"u%d" % w, ("in_seq", 9), w) for w in range(40)]
    cmds = [Cmd(i % 40, 10 + i // 40, 1, 9 + i // 40, 10 + i // 40, 3, b"") for i in range(n)]
    max_size = 26 * k                      # accounted size in front of k: 26 k (not greater); real: 27 k (greater)
    assert 27 * k > max_size >= 26 * k and 26 * (k + 1) > max_size
    return cmds, writers, max_size, k


def check_quirk(be):
    cmds, writers, max_size, k = quirk_case()
    ref, got = run_case(be, np.random.default_rng(3), cmds, writers, next_id_ref=40, max_size=max_size)
    assert all(r[1] and not r[2] for r in ref["rows"][:k + 1])
    assert int(got[0]["status"]) == ROLL and int(got[0]["n_consumed"]) == k + 1
    assert int(got[0]["file_size"]) == 26 * (k + 1) and int(got[0]["out_bytes"]) == 27 * (k + 1)


def test_emu_accounted_size_decides_the_roll(emu):
    check_quirk(emu)


# ------------------------------------------------------------------------------------------ round trip

def check_round_trip(be, checksums):
    rng, cmds, writers, used = fuzz_case(17, 2 * TILE + 3, 19)
    ref, got = run_case(be, rng, cmds, writers, checksums=checksums, next_id_ref=used)
    image = np.frombuffer(abi.WAL_FILE_HEADER + got[3].tobytes(), dtype=np.uint8)
    scanned, consumed, end = be.engine.wal_scan(image)
    assert consumed == len(image) and end == abi.WAL_END_DATA and len(scanned) == ref["n_written"]
    for r, (trunc, id_ref, uid, idx, term, ln), payload in zip(scanned, ref["specs"], ref["payloads"]):
        assert (int(r["index"]), int(r["term"]), int(r["data_len"]), int(r["id_ref"]), int(r["trunc"])) == \
            (idx, term, ln, id_ref, trunc)
        assert bool(int(r["flags"]) & abi.WAL_REC_FIRST) == (uid is not None)
        if uid is not None:
            assert image[int(r["uid_offset"]):int(r["uid_offset"]) + int(r["uid_len"])].tobytes() == uid
        assert image[int(r["data_offset"]):int(r["data_offset"]) + ln].tobytes() == payload
        assert int(r["checksum"]) == (zlib.adler32(struct.pack(">QQ", idx, term) + payload) if checksums else 0)
    # writers named by an earlier batch of this file have short headers only: the scan cannot validate those
    scanned["flags"] |= abi.WAL_REC_VALIDATE
    n_ok, status = be.eng.wal_validate(image, scanned)
    assert (n_ok, status) == (len(scanned), abi.WAL_CLEAN)


@pytest.mark.parametrize("checksums", [True, False], ids=["checksums", "no_checksums"])
def test_emu_round_trip_through_scan_and_validate(emu, checksums):
    check_round_trip(emu, checksums)


# ------------------------------------------------------------------------------------------ framing phases

def check_frame_phases(be, lens, width, out_phase):
    """The payloads of tests/test_wal_framing.py's phase sweep (every length at every source phase) as one command each
    of its own writer, alternately known (3 header bytes) and new (5 + uid); the device form with `out` at out_phase:
    the destination phases follow from the record sizes."""
    rng = np.random.default_rng(99)
    recs, sweep_data, _, _ = phase_sweep_batch(rng, lens, dst_phases=[0])
    n = len(recs)
    uids = [bytes(rng.integers(97, 123, size=int(rng.integers(1, 40)), dtype=np.uint8)) for _ in range(n)]
    uid_at, blob = [], bytearray()
    for u in uids:
        uid_at.append(len(sweep_data) + len(blob))
        blob += u
    data = np.concatenate([sweep_data, np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8)])
    mean = int(recs["data_len"].sum()) // n
    assert {8: mean <= 320, 16: 320 < mean < 1024, 64: mean >= 1024}[width], (width, mean)
    ca = np.zeros(n, dtype=abi.WAL_CMD_DTYPE)
    wa = np.zeros(n, dtype=abi.WAL_WRITER_DTYPE)
    ca["writer"], ca["index"], ca["term"], ca["prev_index"] = np.arange(n), recs["index"], recs["term"], recs["index"] - 1
    ca["tid"], ca["data_offset"], ca["data_len"] = 1, recs["data_offset"], recs["data_len"]
    wa["state"], wa["prev_index"] = IN_SEQ, recs["index"] - 1
    wa["id_ref"] = np.where(np.arange(n) % 2 == 0, np.arange(n), abi.WAL_NO_ID_REF)
    wa["uid_offset"], wa["uid_len"] = uid_at, [len(u) for u in uids]
    fa = np.zeros(1, dtype=abi.WAL_FILE_DTYPE)
    fa["max_size"], fa["next_id_ref"] = BIG, n
    specs, payloads, nxt = [], [], n
    for i in range(n):
        first = i % 2 == 1
        specs.append((0, nxt if first else i, uids[i] if first else None, int(recs["index"][i]), int(recs["term"][i]),
                      int(recs["data_len"][i])))
        nxt += first
        o = int(recs["data_offset"][i])
        payloads.append(data[o:o + int(recs["data_len"][i])].tobytes())
    want = python_frame(specs, payloads)
    out_bound, ev_bound, rg_bound = be.engine.wal_batch_bound(ca, wa, fa, len(data))
    assert out_bound >= len(want)
    data_buf, d_data, _ = be.dev(data, phase=3)             # (kept: the buffer lives as long as its name)
    out_buf, d_out, out_base = be.dev(np.full(out_bound + 64, 0xEE, dtype=np.uint8), phase=out_phase)
    res_buf, d_res, res_base = be.dev(np.zeros(16 * n, dtype=np.uint8))
    wout_buf, d_wout, wout_base = be.dev(np.zeros(32 * n, dtype=np.uint8))
    ev_buf, d_ev, _ = be.dev(np.zeros(32 * ev_bound, dtype=np.uint8))
    rg_buf, d_rg, _ = be.dev(np.zeros(16 * rg_bound, dtype=np.uint8))
    tot_buf, d_tot, tot_base = be.dev(np.zeros(64, dtype=np.uint8))
    be.eng.wal_batch_device(ca, wa, fa, d_data, len(data), d_res, d_wout, d_out, out_bound, d_ev, ev_bound, d_rg, rg_bound,
                            d_tot)
    total = be.get(tot_buf)[tot_base:tot_base + 64].view(abi.WAL_BATCH_TOTAL_DTYPE)[0]
    assert (int(total["status"]), int(total["n_written"]), int(total["out_bytes"])) == (OK, n, len(want))
    got = be.get(out_buf)[out_base:out_base + out_bound + 64].tobytes()
    d = first_diff(got[:len(want)], want)
    assert d is None, d
    assert got[len(want):] == b"\xEE" * (out_bound + 64 - len(want)), "bytes behind the records were written"
    res = be.get(res_buf)[res_base:res_base + 16 * n].view(abi.WAL_CMD_RESULT_DTYPE)
    assert [int(c) for c in res["checksum"]] == \
        [zlib.adler32(struct.pack(">QQ", s[3], s[4]) + p) for s, p in zip(specs, payloads)]


PHASE_SETS = {8: SWEEP_SMALL, 16: SWEEP_MID, 64: SWEEP_LARGE}


@pytest.mark.parametrize("width", [8, 16, 64])
def test_emu_frame_every_source_phase(emu, width):
    check_frame_phases(emu, PHASE_SETS[width][::2], width, out_phase=5)


# ------------------------------------------------------------------------------------------ edges

def small_case():
    writers = [Writer(b"alpha", ("in_seq", 4), 2), Writer(b"b" * 200, None, None), Writer(b"c", ("out_of_seq", 7), None)]
    cmds = [Cmd(0, 5, 1, 4, 0, 1, b"five"), Cmd(1, 1, 1, 0, 0, 2, b""), Cmd(2, 9, 1, 8, 0, 3, b"ignored"),
            Cmd(0, 6, 2, 5, 0, 1, b"six" * 30), Cmd(2, 8, 1, 7, 0, 3, b"eight"), Cmd(1, 2, 1, 1, 0, 2, b"two")]
    return cmds, writers


def check_refusals(be):
    """Every refusal leaves the outputs as they were."""
    cmds, writers = small_case()
    rng = np.random.default_rng(1)
    ca, wa, fa, data = pack(rng, cmds, writers, next_id_ref=3)

    def refused(ca=ca, wa=wa, fa=fa, data_len=len(data), flags=0):
        ca, wa, fa = ca.copy(), wa.copy(), fa.copy()
        with pytest.raises(RgbError) as e:
            be.engine.wal_batch_bound(ca, wa, fa, data_len)
        assert e.value.code == E_INVAL
        bufs = [be.dev(np.full(sz, 0xEE, dtype=np.uint8)) for sz in (16 * len(ca), 32 * len(wa), 4096, 32 * 8, 16 * 8, 64)]
        data_buf, d_data, _ = be.dev(data)
        with pytest.raises(RgbError) as e:
            be.eng.wal_batch_device(ca, wa, fa, d_data, data_len, bufs[0][1], bufs[1][1], bufs[2][1], 4096, bufs[3][1], 8,
                                    bufs[4][1], 8, bufs[5][1], flags=flags)
        assert e.value.code == E_INVAL
        for buf, _, _ in bufs:
            assert bytes(be.get(buf).tobytes()).count(0xEE) >= len(buf) - 32, "a refused call wrote"
        with pytest.raises(RgbError) as e:
            be.eng.wal_batch(ca, wa, fa, data[:data_len], flags=flags, out_bytes=4096, events_cap=8, ranges_cap=8)
        assert e.value.code == E_INVAL

    def changed(arr, field, i, v):
        a = arr.copy()
        a[field][i] = v
        return a

    refused(ca=changed(ca, "writer", 2, 3))                                   # a slot >= W
    refused(ca=changed(ca, "data_offset", 0, len(data) - 1))                  # a payload that ends outside
    refused(ca=changed(ca, "data_offset", 0, (1 << 64) - 2))                  # ... and one whose end wraps around
    refused(wa=changed(wa, "uid_offset", 1, (1 << 64) - 100))
    refused(wa=changed(wa, "uid_len", 1, 65536), data_len=len(data))
    refused(wa=changed(wa, "state", 0, 3))
    refused(wa=changed(wa, "id_ref", 0, 1 << 22))
    refused(fa=changed(fa, "next_id_ref", 0, (1 << 22) - 1))                  # two writers still want an IdRef
    with pytest.raises(RgbError) as e:                                        # unknown flags (the bound takes none)
        be.eng.wal_batch(ca, wa, fa, data, flags=2)
    assert e.value.code == E_INVAL
    L = be.engine.lib()
    assert L.rgb_wal_batch_bound(None, 1, wa.ctypes.data, 3, fa.ctypes.data, 10, None, None, None) == E_INVAL
    assert L.rgb_wal_batch(be.eng._h, ca.ctypes.data, len(ca), wa.ctypes.data, len(wa), None, data.ctypes.data, len(data),
                           0, None, None, None, 0, None, 0, None, 0, None) == E_INVAL


def check_space_and_sizing(be):
    cmds, writers = small_case()
    rng = np.random.default_rng(2)
    ca, wa, fa, data = pack(rng, cmds, writers, next_id_ref=3)
    ref = referee(cmds, writers, 0, 0, 3, BIG, 0)
    sized = be.eng.wal_batch(ca, wa, fa, data, out_bytes=0, events_cap=0, ranges_cap=0)
    t = sized[0]
    assert int(t["status"]) == SPACE and sized[3] is None and sized[4] is None
    assert (int(t["out_bytes"]), int(t["n_events"])) == (len(ref["out"]), len(ref["events"]))
    exact = be.eng.wal_batch(ca, wa, fa, data, out_bytes=int(t["out_bytes"]), events_cap=int(t["n_events"]),
                             ranges_cap=int(t["n_ranges"]))
    check_against(ref, exact, len(writers))
    assert sized[1].tobytes() == exact[1].tobytes() and sized[2].tobytes() == exact[2].tobytes()
    for f in ("n_consumed", "n_written", "n_events", "n_ranges", "next_id_ref", "out_bytes", "file_size", "entry_count"):
        assert int(sized[0][f]) == int(exact[0][f]), f
    # one byte short: SPACE, but the events fit and are delivered
    short = be.eng.wal_batch(ca, wa, fa, data, out_bytes=int(t["out_bytes"]) - 1, events_cap=int(t["n_events"]),
                             ranges_cap=int(t["n_ranges"]))
    assert int(short[0]["status"]) == SPACE and short[3] is None
    assert events_of(short[4], short[5]) == ref["events"]
    # one pair short
    short = be.eng.wal_batch(ca, wa, fa, data, out_bytes=int(t["out_bytes"]), events_cap=int(t["n_events"]),
                             ranges_cap=int(t["n_ranges"]) - 1)
    assert int(short[0]["status"]) == SPACE and short[4] is None


def check_empty_and_roll_at_zero(be):
    cmds, writers = small_case()
    rng = np.random.default_rng(4)
    ca, wa, fa, data = pack(rng, [], writers, file_size=77, entry_count=5, next_id_ref=3)
    t, results, wout, out, events, ranges = be.eng.wal_batch(ca, wa, fa, data)
    assert (int(t["status"]), int(t["n_consumed"]), int(t["out_bytes"]), int(t["file_size"]), int(t["entry_count"]),
            int(t["next_id_ref"]), len(events)) == (OK, 0, 0, 77, 5, 3, 0)
    assert wout.tobytes() == wa.tobytes()
    t = be.eng.wal_batch(np.zeros(0, abi.WAL_CMD_DTYPE), np.zeros(0, abi.WAL_WRITER_DTYPE), fa, np.zeros(0, np.uint8))[0]
    assert int(t["status"]) == OK
    # the file is already over its size: command 0 rolls, nothing is consumed, the writers are as they came
    ref, got = run_case(be, rng, cmds, writers, file_size=1001, next_id_ref=3, max_size=1000)
    assert (ref["status"], ref["n_consumed"]) == (ROLL, 0) and len(got[3]) == 0 and len(got[4]) == 0
    # a DROP in front of the first WRITE is consumed before the roll
    cmds2 = [Cmd(0, 3, 1, 2, 5, 1, b"dropped")] + cmds
    ref, got = run_case(be, rng, cmds2, writers, file_size=1001, next_id_ref=3, max_size=1000)
    assert (ref["status"], ref["n_consumed"]) == (ROLL, 1)


def check_resume_after_roll(be):
    """The caller's loop: write, roll, call again from n_consumed with a fresh file and no writer named in it."""
    rng, cmds, writers, used = fuzz_case(17, 2 * TILE + 3, 19)
    max_entries = 150
    files, pos, ws = [], 0, writers
    while pos < len(cmds):
        ref, got = run_case(be, rng, cmds[pos:], ws, next_id_ref=used if not files else 0, max_entries=max_entries)
        files.append(got[3].tobytes())
        assert ref["n_consumed"] > 0
        pos += ref["n_consumed"]
        wout = got[2]
        ws = [Writer(w.uid, None if int(r["state"]) == UNDEFINED else
                     ("in_seq" if int(r["state"]) == IN_SEQ else "out_of_seq", int(r["prev_index"])), None)
              for w, r in zip(writers, wout)]
    assert len(files) >= 3
    # the whole mailbox through the referee alone, rolling as the reference does
    ref_files, pos, ws, nxt = [], 0, writers, used
    while pos < len(cmds):
        ref = referee(cmds[pos:], ws, 0, 0, nxt, BIG, max_entries)
        ref_files.append(ref["out"])
        pos += ref["n_consumed"]
        ws = [Writer(w.uid, st, None) for w, (st, _) in zip(writers, ref["writers"])]
        nxt = 0
    assert files == ref_files


def check_id_ref_ceiling(be):
    top = (1 << 22) - 1
    writers = [Writer(b"known", ("in_seq", 1), top), Writer(b"new", None, None)]
    cmds = [Cmd(0, 2, 1, 1, 0, 1, b"a"), Cmd(1, 1, 1, 0, 0, 1, b"b"), Cmd(1, 2, 1, 1, 2, 1, b"c")]
    ref, got = run_case(be, np.random.default_rng(6), cmds, writers, next_id_ref=top)
    assert int(got[0]["next_id_ref"]) == 1 << 22 and int(got[2]["id_ref"][1]) == top
    assert got[3].tobytes()[:3] == bytes([0x7F, 0xFF, 0xFF])


def check_wide_values(be):
    for base in BASES[1:]:
        writers = [Writer(b"w", ("in_seq", base), 0)]
        cmds = [Cmd(0, base + 1 + i, base + i // 2, base + i, base + 3 if i >= 2 else 0, (1 << 64) - 1 - i // 3, b"p" * i)
                for i in range(6)]
        cmds.append(Cmd(0, base + 9, base, base + 8, 0, 5, b""))              # a gap behind them
        run_case(be, np.random.default_rng(7), cmds, writers, next_id_ref=1, file_size=(1 << 62), max_size=(1 << 63))


EDGE_CHECKS = {"refusals": check_refusals, "space_and_sizing": check_space_and_sizing,
               "empty_and_roll_at_zero": check_empty_and_roll_at_zero, "resume_after_roll": check_resume_after_roll,
               "id_ref_ceiling": check_id_ref_ceiling, "wide_values": check_wide_values}


@pytest.mark.parametrize("name", list(EDGE_CHECKS))
def test_emu_edges(emu, name):
    EDGE_CHECKS[name](emu)


def test_abi_mirror():
    """The dtypes of ra_amd/abi.py against the sizes the header's structs have in a C compiler's eyes."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = ('#include <stdio.h>\n#include "ra_gpu_wal.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", '
           "sizeof(rgb_wal_cmd), sizeof(rgb_wal_writer), sizeof(rgb_wal_file), sizeof(rgb_wal_cmd_result), "
           "sizeof(rgb_wal_event), sizeof(rgb_wal_batch_total)); return 0;}")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "s.c"), os.path.join(tmp, "s")
        with open(c, "w") as f:
            f.write(src)
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", exe, c])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [d.itemsize for d in (abi.WAL_CMD_DTYPE, abi.WAL_WRITER_DTYPE, abi.WAL_FILE_DTYPE,
                                          abi.WAL_CMD_RESULT_DTYPE, abi.WAL_EVENT_DTYPE, abi.WAL_BATCH_TOTAL_DTYPE)]


# ------------------------------------------------------------------------------------------ host helpers, sanitized

def test_host_helpers_under_sanitizers(tmp_path):
    """rgb_wal_host.cpp's validation, per-writer order and bound in a stand-alone program (tests/native/
    wal_batch_harness.cpp) under ASan and UBSan: no Python, no preloaded runtime."""
    cxx = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "wal_batch_harness"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "native", "wal_batch_harness.cpp"),
                            os.path.join(ROOT, "ra_amd", "csrc", "rgb_wal_host.cpp")], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this compiler has no sanitizer runtime: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert "wal batch harness ok" in run.stdout


# ------------------------------------------------------------------------------------------ resources

# kernel -> the instances it is built in (lanes per writer / per record: 8, 16, 64)
NEW_KERNELS = {"rgb_wal_batch_verdict_kernel": 3, "rgb_wal_batch_sum_kernel": 1, "rgb_wal_batch_place_kernel": 1,
               "rgb_wal_batch_rows_kernel": 1, "rgb_wal_batch_events_kernel": 3, "rgb_wal_batch_gather_kernel": 1,
               "rgb_wal_batch_frame_kernel": 3}


def wal_kernel_resources():
    """hipcc's resource-usage remarks for every kernel of rgb_wal.hip on gfx950, parsed as tests/test_kernel_resources.py
    parses them for the segment unit: {mangled name: {remark: value}}"""
    from test_kernel_resources import HIPCC, _parse
    if HIPCC is None:
        pytest.skip("no hipcc")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-mllvm",
                        "-disable-machine-licm", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(ROOT, "ra_amd", "csrc", "rgb_wal.hip"), "-o", os.devnull],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return _parse(r.stderr)


def test_new_kernels_use_no_scratch():
    res = wal_kernel_resources()
    for k, instances in NEW_KERNELS.items():
        mine = {n: v for n, v in res.items() if k in n}
        assert len(mine) == instances, (k, sorted(res))
        for n, v in mine.items():
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, f"{n} spills to scratch: {v}"


# ------------------------------------------------------------------------------------------ GPU twins

@pytest.mark.gpu
@pytest.mark.parametrize("n,n_writers,seed", FUZZ_SHAPES)
def test_gpu_referee_parity(gpu, n, n_writers, seed):
    check_fuzz(gpu, n, n_writers, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("case_name", GOLDEN_NAMES)
def test_gpu_reference_suite_outcomes(gpu, case_name):
    check_golden(gpu, case_name)


@pytest.mark.gpu
def test_gpu_accounted_size_decides_the_roll(gpu):
    check_quirk(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("checksums", [True, False], ids=["checksums", "no_checksums"])
def test_gpu_round_trip_through_scan_and_validate(gpu, checksums):
    check_round_trip(gpu, checksums)


@pytest.mark.gpu
@pytest.mark.parametrize("out_phase", [0, 5, 11])
@pytest.mark.parametrize("width", [8, 16, 64])
def test_gpu_frame_every_source_phase(gpu, width, out_phase):
    check_frame_phases(gpu, PHASE_SETS[width], width, out_phase)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDGE_CHECKS))
def test_gpu_edges(gpu, name):
    EDGE_CHECKS[name](gpu)
