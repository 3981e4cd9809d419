"""Major compaction on the device: rgb_segment_info* and rgb_segment_compact* (include/ra_gpu_wal.h, "major
compaction"; ra_amd/csrc/rgb_segment.hip, rgb_segment_host.cpp).

Referee: three pure-Python functions written from the reference source, sequentially, with a dict --
  ref_parse    parse_index_data_loop   src/ra_log_segment.erl:1057-1075 (maps:filter on a backwards step)
  ref_info     parse_index_info_loop   src/ra_log_segment.erl:1084-1116 (+ info/2, :736-790)
  ref_compact  copy/3 + append_raw/6   src/ra_log_segment.erl:819-908, is_full/1 :1250-1255, for the sources of a group
                                       in the caller's order (src/ra_log_segments.erl:792-802)
-- plus struct.pack and zlib.crc32.  The library computes "which records are in the final map" as a reverse min-scan;
the referee deliberately does not.  Two things the reference does not do are defined by include/ra_gpu_wal.h and
restated in ref_compact: a selected record whose payload lies outside its file is TRUNCATED (the reference's pread
would come back short), and with the VERIFY flag the first copied payload that does not match a non-zero stored Crc is
reported when nothing else is wrong.  Source images are packed by hand, in the record order a test wants.

Every device check exists twice: on the CPU emulation of the same sources (-m "not gpu") and on the GPU."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from emu_schedule import PERMUTED_SCHEDULES, schedule
from ra_amd import abi
from test_segment import Emu, Gpu, emu, gpu, first_diff, python_segment          # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL = -1
OK, MISSING, FULL, TRUNCATED, SPACE, CRC, BAD_SOURCE = range(7)
VERIFY = abi.SEG_COMPACT_VERIFY
MAX_SIZE = abi.SEG_MAX_SIZE_B
CHUNK = 256                    # rgb_segment.hip: records per step of the resolve pass (one workgroup)
GUARD = 64


# ------------------------------------------------------------------------------------------ referee

def _walk(f: bytes):
    """decode_index_record/3 over file:pread(Fd, 8, IndexSize): (Idx, Term, Offset, Length, Crc) until eof."""
    version, max_count = struct.unpack(">HH", f[4:8])
    rec, fmt = (32, ">QQQII") if version == 2 else (28, ">QQIII")
    region = f[8:8 + max_count * rec]
    pos = 0
    while len(region) >= pos + rec:
        r = struct.unpack(fmt, region[pos:pos + rec])
        if r == (0, 0, 0, 0, 0):
            return
        yield r
        pos += rec


def _data_start(f: bytes) -> int:
    version, max_count = struct.unpack(">HH", f[4:8])
    return 8 + max_count * (32 if version == 2 else 28)


def ref_parse(f: bytes) -> dict:
    index, last_idx = {}, 0
    for idx, term, offset, length, crc in _walk(f):
        if idx < last_idx:                                  # trim index entries if Idx goes "backwards"
            index = {k: v for k, v in index.items() if not k > idx}
        index[idx] = (term, offset, length, crc)
        last_idx = idx
    return index


def _in_seq(idx, live):
    return any(a <= idx <= b for a, b in live)


def ref_info(f: bytes, live):
    """live: None (undefined) or a list of (first, last)."""
    num, last_idx, data_offset, rng, idx_acc, live_size = 0, 0, _data_start(f), None, [], 0
    for idx, _term, offset, length, _crc in _walk(f):
        if idx < last_idx:
            while idx_acc and idx_acc[-1] > idx:             # lists:dropwhile over the head of the accumulator
                idx_acc.pop()
        if live is None or _in_seq(idx, live):
            live_size += length
        num, last_idx, data_offset = num + 1, idx, offset + length
        rng = (idx, idx) if rng is None else (min(rng[0], idx), idx)
        idx_acc.append(idx)
    version, max_count = struct.unpack(">HH", f[4:8])
    return dict(num_entries=num, size=data_offset, index_size=_data_start(f), range=rng, live_size=live_size,
                indexes=sorted(set(idx_acc)), max_count=max_count, version=version)       # ra_seq:from_list usorts


def _expand(live):
    return [i for a, b in live for i in range(a, b + 1)]


def _bad_header(f: bytes) -> bool:
    return len(f) < 8 or f[:4] != b"RASG" or struct.unpack(">H", f[4:6])[0] not in (1, 2)


def ref_compact(files, lives, max_size=MAX_SIZE, verify=False):
    """-> the image bytes, or (status, source, index)."""
    for s, f in enumerate(files):                           # info/2 of every file comes first and would crash
        if _bad_header(f):
            return (BAD_SOURCE, s, 0)
    max_count = sum(len(_expand(l)) for l in lives)
    data_start = 8 + 32 * max_count
    data_offset, index, payloads, copied = data_start, [], [], []
    for s, (f, live) in enumerate(zip(files, lives)):
        src = ref_parse(f)
        for idx in sorted(_expand(live)):
            if idx not in src:
                return (MISSING, s, idx)                    # exit({copy_missing_key, Idx})
            term, pos, length, crc = src[idx]
            if pos + length > len(f):
                return (TRUNCATED, s, idx)
            data = f[pos:pos + length]
            if data_offset - data_start > max_size:         # is_full/1: "greater than"
                return (FULL, s, idx)
            index.append(struct.pack(">QQQII", idx, term, data_offset, length, crc))
            payloads.append(data)
            copied.append((s, idx, crc))
            data_offset += length
    if verify:
        for (s, idx, crc), data in zip(copied, payloads):
            if crc != 0 and zlib.crc32(data) != crc:        # validate_checksum/2: 0 = not checked
                return (CRC, s, idx)
    return struct.pack(">4sHH", b"RASG", 2, max_count) + b"".join(index) + bytes(32 * (max_count - len(index))) + \
        b"".join(payloads)


# ------------------------------------------------------------------------------------------ building inputs

def R(idx, term, payload=b"", crc=None, gap=0, off=None, ln=None):
    return dict(idx=idx, term=term, payload=payload, crc=crc, gap=gap, off=off, ln=ln)


def make_source(recs, max_count=None, version=2, tail=0) -> bytes:
    """A segment image packed by hand: the index records in the order given, payloads back to back behind the index
    region (`gap` filler bytes in front of one, `off` / `ln` to make a record point elsewhere)."""
    rec, fmt = (32, ">QQQII") if version == 2 else (28, ">QQIII")
    mc = len(recs) if max_count is None else max_count
    assert mc >= len(recs)
    pos, index, body = 8 + mc * rec, [], []
    for r in recs:
        body.append(b"\x5a" * r["gap"]); pos += r["gap"]
        crc = zlib.crc32(r["payload"]) if r["crc"] is None else r["crc"]
        index.append(struct.pack(fmt, r["idx"], r["term"], pos if r["off"] is None else r["off"],
                                 len(r["payload"]) if r["ln"] is None else r["ln"], crc))
        body.append(r["payload"]); pos += len(r["payload"])
    return struct.pack(">4sHH", b"RASG", version, mc) + b"".join(index) + bytes(rec * (mc - len(recs))) + \
        b"".join(body) + b"\x3c" * tail


def ranges_of(indexes):
    out = []
    for i in sorted(set(indexes)):
        if out and i == out[-1][1] + 1:
            out[-1][1] = i
        else:
            out.append([i, i])
    return [tuple(r) for r in out]


def pack_group(files, lives, gaps=None):
    buf, live = bytearray(), []
    sources = np.zeros(len(files), dtype=abi.SEG_SOURCE_DTYPE)
    for s, f in enumerate(files):
        buf += b"\xa5" * (gaps[s] if gaps else 3 * s + 1)
        sources["offset"][s], sources["n_bytes"][s] = len(buf), len(f)
        if lives is not None:
            sources["live_first"][s], sources["live_n"][s] = len(live), len(lives[s])
            live += lives[s]
        buf += f
    buf += b"\xa5" * 5
    live_arr = None if lives is None else np.array(live, dtype=np.uint64).reshape(-1, 2)
    return sources, np.frombuffer(bytes(buf), dtype=np.uint8).copy(), live_arr


def rnd_payloads(rng, n, hi=25):
    return [rng.integers(0, 256, size=int(ln), dtype=np.uint8).tobytes() for ln in rng.integers(0, hi, size=n)]


def source_of(rng, idxs, **kw):
    """records with the given Idx sequence, a distinct Term each, small random payloads"""
    pay = rnd_payloads(rng, len(idxs))
    return make_source([R(i, j + 1, p) for j, (i, p) in enumerate(zip(idxs, pay))], **kw)


def pad_to_width(files, max_count, width):
    """Lengthen the last file (bytes behind its payloads) until (sum of n_bytes) / max(1, MaxCount) selects the
    lane-group width: 8 lanes up to 320, 16 below 1024, else a wavefront -- the rule of rgb_segment_compact_device."""
    files = list(files)
    n, total = max(1, max_count), sum(len(f) for f in files)
    want = {8: 0, 16: 600, 64: 1100}[width] * n
    if total < want:
        files[-1] = files[-1] + b"\x3c" * (want - total)
    mean = sum(len(f) for f in files) // n
    assert {8: mean <= 320, 16: 320 < mean < 1024, 64: mean >= 1024}[width], (width, mean)
    return files


# ------------------------------------------------------------------------------------------ calling the library

def prepared_compact(be, sources, buf, live, max_size=MAX_SIZE, flags=0, out_bytes=None, src_phase=0, dst_phase=0):
    """-> (call, fetch): the buffers of one rgb_segment_compact_device call are on the device; call() enqueues it,
    fetch() waits and returns what device_compact returns."""
    if out_bytes is None:
        out_bytes = be.engine.segment_compact_bound(sources, live, len(buf))[0] + 48
    arr = np.concatenate([np.full(GUARD, 0xC3, dtype=np.uint8), np.full(out_bytes, 0xEE, dtype=np.uint8),
                          np.full(GUARD, 0xC3, dtype=np.uint8)])
    d_f, p_f, _ = be.dev(buf, src_phase)
    d_o, p_o, b_o = be.dev(arr, dst_phase)
    d_r, p_r, b_r = be.dev(np.full(32, 0x77, dtype=np.uint8))

    def call():
        be.eng.segment_compact_device(sources, p_f, len(buf), live, p_o + GUARD, out_bytes, p_r, max_size, flags)

    def fetch(_keep=d_f):                                   # (the source buffer lives until the answer has been read)
        got = be.get(d_o)
        res = be.get(d_r)[b_r:b_r + 32].copy().view(abi.SEG_COMPACT_RESULT_DTYPE)[0]
        assert np.all(got[:b_o] == 0) and np.all(got[b_o + len(arr):] == 0), "wrote outside the buffer"
        assert np.all(got[b_o:b_o + GUARD] == 0xC3), "wrote in front of d_out"
        assert np.all(got[b_o + GUARD + out_bytes:b_o + len(arr)] == 0xC3), "wrote behind d_out"
        return res, got[b_o + GUARD:b_o + GUARD + out_bytes].copy()
    return call, fetch


def device_compact(be, sources, buf, live, max_size=MAX_SIZE, flags=0, out_bytes=None, src_phase=0, dst_phase=0):
    """-> (result record, the out_bytes of d_out); guard bytes in front of and behind d_out are checked."""
    call, fetch = prepared_compact(be, sources, buf, live, max_size, flags, out_bytes, src_phase, dst_phase)
    call()
    return fetch()


def check_group(be, files, lives, max_size=MAX_SIZE, flags=0, src_phase=0, dst_phase=0, host_form=True, what=""):
    """Both forms against the referee: the image byte for byte, or the status with its source and index."""
    want = ref_compact(files, lives, max_size, bool(flags & VERIFY))
    sources, buf, live = pack_group(files, lives)
    bound, max_count = be.engine.segment_compact_bound(sources, live, len(buf))
    assert max_count == sum(len(_expand(l)) for l in lives) and bound == 8 + 32 * max_count + sum(len(f) for f in files)
    res, region = device_compact(be, sources, buf, live, max_size, flags, None, src_phase, dst_phase)
    if isinstance(want, bytes):
        assert int(res["status"]) == OK, f"{what}: status {int(res['status'])} source {int(res['source'])} index {int(res['index'])}"
        assert (int(res["n_entries"]), int(res["file_bytes"])) == (max_count, len(want)), what
        diff = first_diff(region[:len(want)].tobytes(), want)
        assert diff is None, f"{what}: {diff}"
        assert np.all(region[len(want):] == 0xEE), f"{what}: bytes behind file_bytes were written"
    else:
        assert (int(res["status"]), int(res["source"]), int(res["index"])) == want, what
    if host_form:
        out = np.full(bound + 40, 0xEE, dtype=np.uint8)
        if not isinstance(want, bytes) and want[0] == BAD_SOURCE:
            with pytest.raises(be.engine.RgbError) as e:
                be.eng.segment_compact(sources, buf, live, max_size, flags, out=out)
            assert e.value.code == E_INVAL and np.all(out == 0xEE)
            return want
        res, image = be.eng.segment_compact(sources, buf, live, max_size, flags, out=out)
        if isinstance(want, bytes):
            assert int(res["status"]) == OK and first_diff(image.tobytes(), want) is None, what
            assert np.all(out[len(want):] == 0xEE), f"{what}: bytes of out behind file_bytes were written"
        else:
            assert (int(res["status"]), int(res["source"]), int(res["index"])) == want and image is None, what
            assert np.all(out == 0xEE), f"{what}: out was written although the status is not OK"
    return want


def check_info(be, files, lives, what=""):
    sources, buf, live = pack_group(files, lives)
    d_f, p_f, _ = be.dev(buf, 5)
    d_i, p_i, b_i = be.dev(np.full(64 * len(files), 0x77, dtype=np.uint8))
    be.eng.segment_info_device(sources, p_f, len(buf), live, p_i)
    rows_dev = be.get(d_i)[b_i:b_i + 64 * len(files)].copy().view(abi.SEG_INFO_DTYPE)
    rows_host = be.eng.segment_info(sources, buf, live)
    for rows in (rows_dev, rows_host):
        for s, f in enumerate(files):
            want, got = ref_info(f, None if lives is None else lives[s]), rows[s]
            tag = f"{what} source {s}"
            assert int(got["status"]) == OK, tag
            for k in ("num_entries", "size", "index_size", "live_size", "max_count", "version"):
                assert int(got[k]) == want[k], f"{tag}: {k} {int(got[k])} != {want[k]}"
            assert int(got["num_indexes"]) == len(want["indexes"]) == len(ref_parse(f)), tag
            if want["range"] is not None:
                assert (int(got["range_first"]), int(got["range_last"])) == want["range"], tag


# ------------------------------------------------------------------------------------------ the checks

def scan_patterns(n, rng):
    """Idx sequences of n records: ascending; one backwards step exactly at, before and behind every chunk boundary of
    the resolve pass; an equal neighbour (an overwrite, not a trim); a late record lower than everything; random walks."""
    base = list(range(100, 100 + n))
    pats = [("ascending", base)]
    for edge in range(CHUNK, n + CHUNK, CHUNK):
        for p in (edge - 1, edge, edge + 1):
            if 1 <= p < n:
                seq = base[:p] + [base[p - 1] - min(3, p) + k for k in range(n - p)]
                pats.append((f"backwards_at_{p}", seq))
    if n >= 2:
        p = n // 2
        pats.append(("equal_neighbour", base[:p] + [base[p - 1] + k for k in range(n - p)]))
        pats.append(("first_pair_backwards", [base[1], base[0]] + base[2:]))
        pats.append(("late_low", base[:-1] + [1]))
    for w in range(3):
        seq, cur = [], 50
        for step in rng.integers(-6, 5, size=n):
            cur = max(1, cur + int(step))
            seq.append(cur)
        pats.append((f"walk_{w}", seq))
    return pats


SCAN_SIZES = [1, 2, 255, 256, 257, 1000]      # 1000: more than three chunks of the workgroup


def check_effective_scan(be, n):
    rng = np.random.default_rng(500 + n)
    pats = scan_patterns(n, rng)
    names = ", ".join(p[0] for p in pats)
    files = [source_of(rng, seq) for _, seq in pats]
    if n == 1000:
        assert len(ref_parse(files[-1])) < 500 and any(len(ref_parse(f)) == 1 for f in files)     # the walks do trim
    live_all = [ranges_of(ref_parse(f).keys()) for f in files]
    live_some = [ranges_of(k for k in ref_parse(f) if k % 3) for f in files]
    check_info(be, files, None, f"n {n}, no live list ({names})")
    check_info(be, files, live_some, f"n {n}, some live")
    for lives in (live_all, live_some):
        want = check_group(be, files, lives, what=f"n {n} ({names})")
        assert isinstance(want, bytes)


def check_scan_width(be):
    """One source with MaxCount = 65535 records (the widest index the header can state), payloads of 0 to 3 bytes,
    backwards steps far apart so that the minimum has to travel across many chunks."""
    rng = np.random.default_rng(510)
    n = 65535
    idxs = np.arange(1000, 1000 + n)
    for p, back in ((70, 50), (20001, 9000), (40000, 1), (65000, 30000)):
        idxs[p:] = idxs[p - 1] - back + np.arange(n - p)
    lens = rng.integers(0, 4, size=n)
    blob = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8).tobytes()
    ends = np.cumsum(lens)
    recs = [R(int(i), 3, blob[int(e - ln):int(e)]) for i, ln, e in zip(idxs, lens, ends)]
    f = make_source(recs)
    keys = sorted(ref_parse(f))
    assert 1000 < len(keys) < n
    check_info(be, [f], [ranges_of(keys)], "MaxCount 65535")
    want = check_group(be, [f], [ranges_of(keys)], host_form=False, what="MaxCount 65535")
    assert isinstance(want, bytes) and sorted(ref_parse(want)) == keys


def check_versions_and_walk_ends(be):
    rng = np.random.default_rng(520)
    pay = rnd_payloads(rng, 40, 60)
    recs = [R(10 + j, 2, p) for j, p in enumerate(pay)]
    v1 = make_source(recs, max_count=64, version=1)
    v2 = make_source([R(60 + j, 3, p) for j, p in enumerate(pay)], max_count=40)
    assert v1 == python_segment([(10 + j, 2) for j in range(40)], pay, 64, version=1)         # a well-formed source
    # an all-zero record in the middle ends the walk: the records behind it do not exist
    holed = bytearray(make_source(recs)); holed[8 + 32 * 17:8 + 32 * 18] = bytes(32)
    # MaxCount smaller than the records present: MaxCount records are read
    short = bytearray(make_source(recs)); short[6:8] = struct.pack(">H", 25)
    # the file ends inside the index region: whole records in front of the end are walked, their payloads are gone
    cut = make_source(recs)[:8 + 32 * 9 + 11]
    empty = make_source([], max_count=16)
    header_only = make_source([], max_count=16)[:8]
    files = [v1, v2, bytes(holed), bytes(short), cut, empty, header_only]
    assert [len(ref_parse(f)) for f in files] == [40, 40, 17, 25, 9, 0, 0]
    check_info(be, files, None, "walk ends")
    lives = [ranges_of(ref_parse(f).keys()) for f in files]
    check_info(be, files, lives, "walk ends, live")
    lives[4] = []                                           # (its payloads lie behind the cut: see check_statuses)
    want = check_group(be, files, lives, what="version 1 + version 2")
    assert isinstance(want, bytes) and want[4:6] == b"\x00\x02"
    assert check_group(be, files[:4] + [cut], lives[:4] + [[(10, 10)]])[0] == TRUNCATED


def check_live_slices(be):
    rng = np.random.default_rng(530)
    eff = list(range(10, 21)) + list(range(30, 36)) + [50]
    a = source_of(rng, [7, 8, 9, 40, 41] + eff[:5] + [99, 100] + eff[5:])        # 40, 41, 99, 100 are trimmed away
    b = source_of(rng, list(range(200, 230)))
    assert sorted(ref_parse(a)) == [7, 8, 9] + eff
    for name, la, lb in (("empty slice", [], [(200, 229)]),
                         ("single index", [(30, 30)], []),
                         ("first and last effective", [(7, 20), (30, 35), (50, 50)], [(200, 200), (229, 229)]),
                         ("all live", ranges_of(ref_parse(a)), ranges_of(ref_parse(b))),
                         ("every other", [(i, i) for i in eff[::2]], [(i, i) for i in range(200, 230, 2)]),
                         ("none live", [], [])):
        want = check_group(be, [a, b], [la, lb], what=name)
        assert isinstance(want, bytes), name
        if name == "none live":
            assert want == b"RASG\x00\x02\x00\x00"
    # ranges whose ends fall between effective indexes hold indexes that are not there: the referee's verdict
    for la in ([(10, 22)], [(28, 35)], [(36, 50)], [(1, 9)]):
        assert check_group(be, [a, b], [la, [(200, 210)]], what=str(la))[0] == MISSING
    check_info(be, [a, b], [[(9, 31)], []], "live ends between effective indexes")


def check_same_index_in_two_sources(be):
    rng = np.random.default_rng(540)
    old = source_of(rng, list(range(1, 40)))
    new = make_source([R(i, 9, bytes([i]) * (i % 11)) for i in range(30, 60)])
    want = check_group(be, [old, new], [[(1, 39)], [(30, 59)]], what="same index live twice")
    assert isinstance(want, bytes)
    merged = ref_parse(want)                                # the new file's own index goes backwards: the newer wins
    assert sorted(merged) == list(range(1, 60)) and all(merged[i][0] == 9 for i in range(30, 60))
    assert len(list(_walk(want))) == 39 + 30


def check_stored_crc_zero(be):
    rng = np.random.default_rng(550)
    pay = rnd_payloads(rng, 12, 300)
    pay[0] = bytes(range(50))
    f = make_source([R(5 + j, 1, p, crc=0 if j % 3 == 0 else None) for j, p in enumerate(pay)])
    damaged = bytearray(f); damaged[_data_start(f) + 1] ^= 0x40           # inside payload 0, whose stored Crc is 0
    for flags in (0, VERIFY):
        for img in (f, bytes(damaged)):
            want = check_group(be, [img], [[(5, 16)]], flags=flags, what=f"stored crc 0, flags {flags}")
            assert isinstance(want, bytes) and want[8 + 28:8 + 32] == bytes(4)


def check_back_to_back_calls(be):
    """Two calls of the device form on a fresh context with nothing waited for in between.  The first (one source, one
    live range) leaves a pinned descriptor block of 160 bytes and a device copy of 4216; the second has 320
    single-index live ranges at 20 bytes each, so both blocks are regrown while the first call's upload and kernels
    may still be under way.  Only the GPU half has anything in flight: the emulation runs each call to its end, and
    there this checks the regrowth alone.  The sizes are those of rgb_segment.hip's growth rules (pinned: twice the
    need; device: need + need / 2 + 4096) worked out by hand; the library does not report its capacities, so the
    assertion below documents the shapes and does not follow a change of those rules."""
    rng = np.random.default_rng(555)
    groups = [([source_of(rng, [7])], [[(7, 7)]]),
              ([source_of(rng, list(range(100, 740)))], [[(i, i) for i in range(100, 740, 2)]])]
    assert 20 * len(groups[1][1][0]) > max(160, 4216)
    fresh = type(be)(be.engine)
    try:
        runs = [prepared_compact(fresh, *pack_group(files, lives)) for files, lives in groups]
        for call, _ in runs:
            call()
        for (files, lives), (_, fetch) in zip(groups, runs):
            want = ref_compact(files, lives)
            res, region = fetch()
            assert int(res["status"]) == OK and int(res["file_bytes"]) == len(want)
            assert first_diff(region[:len(want)].tobytes(), want) is None
            assert np.all(region[len(want):] == 0xEE), "bytes behind file_bytes were written"
    finally:
        fresh.close()


SHAPE_LENS = [0, 1, 15, 16, 17, 31, 33, 4095, 4096, 4097]


def check_payload_shapes(be, width):
    rng = np.random.default_rng(560 + width)
    more = rng.integers(0, 60, size=300) if width == 8 else rng.integers(0, 700, size=40)   # (keeps the mean in its band)
    lens = SHAPE_LENS + ([65537, 100001] if width == 64 else []) + [int(x) for x in more]
    recs = [R(1 + j, 4, rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes(), gap=int(rng.integers(0, 17)))
            for j, ln in enumerate(lens)]
    a, b = make_source(recs[:20], max_count=32), make_source(recs[20:], version=1)
    files = pad_to_width([a, b], len(lens), width)
    for flags in (0, VERIFY):
        for sp, dp in ((0, 0), (3, 9)):
            want = check_group(be, files, [[(1, 20)], [(21, len(lens))]], flags=flags, src_phase=sp, dst_phase=dp,
                               what=f"width {width} flags {flags} phases {sp}, {dp}")
            assert isinstance(want, bytes)


def check_every_phase(be, width, flags):
    """Lengths 15 to 49 at every source phase x destination phase mod 16.  The destination phase of an entry follows
    from the lengths copied before it: the entries are ordered so that each length meets every phase (a filler entry
    of 1 to 15 bytes only where nothing is left to do at the phase reached); the source phase is set by a gap."""
    rng = np.random.default_rng(570 + width)
    todo = {dp: [(ln, sp) for ln in range(15, 50) for sp in range(16)] for dp in range(16)}
    for dp in todo:
        rng.shuffle(todo[dp])
    recs, dst, src_pos, seen = [], 8, 8, set()           # dst, src_pos: the offsets mod 16 (both index regions are
    while any(todo.values()):                            # multiples of 16 bytes, the header has 8)
        if not todo[dst % 16]:
            fill = next(k for k in range(1, 16) if todo[(dst + k) % 16])
            recs.append(R(len(recs) + 1, 1, rng.integers(0, 256, size=fill, dtype=np.uint8).tobytes()))
            dst, src_pos = dst + fill, src_pos + fill
        ln, sp = todo[dst % 16].pop()
        gap = (sp - src_pos) % 16
        recs.append(R(len(recs) + 1, 2, rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes(), gap=gap))
        src_pos += gap
        seen.add((ln, src_pos % 16, dst % 16))
        dst, src_pos = dst + ln, src_pos + ln
    assert len(seen) == 35 * 256 and len(recs) < 35 * 256 + 600
    files = pad_to_width([make_source(recs)], len(recs), width)
    sources, buf, live = pack_group(files, [[(1, len(recs))]], gaps=[16])
    want = ref_compact(files, [[(1, len(recs))]])
    res, region = device_compact(be, sources, buf, live, MAX_SIZE, flags, None, 0, 0)
    assert int(res["status"]) == OK
    diff = first_diff(region[:len(want)].tobytes(), want)
    assert diff is None, f"width {width} flags {flags}: {diff}"
    assert np.all(region[len(want):] == 0xEE)


def check_statuses(be):
    rng = np.random.default_rng(580)
    a = source_of(rng, [1, 2, 3, 4, 5, 6, 7, 8, 4, 5, 9, 10])              # 6, 7, 8 are trimmed away
    b = source_of(rng, list(range(20, 40)))
    assert sorted(ref_parse(a)) == [1, 2, 3, 4, 5, 9, 10]
    for name, la, lb, want in (("trimmed", [(1, 7)], [(20, 39)], (MISSING, 0, 6)),
                               ("never there", [(1, 5), (9, 12)], [(20, 39)], (MISSING, 0, 11)),
                               ("second source", [(1, 5)], [(20, 25), (38, 45)], (MISSING, 1, 40)),
                               ("both: the first in copy order", [(3, 7)], [(19, 21)], (MISSING, 0, 6))):
        assert check_group(be, [a, b], [la, lb], what=name) == want, name

    # FULL: 100-byte payloads; refused is the first entry with MORE than max_size bytes in front of it
    pay = [bytes([j]) * 100 for j in range(30)]
    s0 = make_source([R(1 + j, 1, p) for j, p in enumerate(pay[:8])])
    s1 = make_source([R(9 + j, 1, p) for j, p in enumerate(pay[8:])])
    group = ([s0, s1], [[(1, 8)], [(9, 30)]])
    for k in (3, 8, 10, 29, 30):
        for d in (-1, 0, 1):
            want = check_group(be, *group, max_size=100 * k + d, what=f"max_size {100 * k + d}")
            refused = k + 1 if d < 0 else k + 2             # the index whose predecessors weigh 100 k (+ 100) bytes
            assert want == (FULL, 0 if refused <= 8 else 1, refused) if refused <= 30 else isinstance(want, bytes), (k, d)
    assert check_group(be, *group, max_size=0)[:1] == (FULL,)
    # a missing index in front of the refused entry wins, one behind it does not
    assert check_group(be, [s0, s1], [[(1, 8)], [(9, 12), (14, 31)]], max_size=2000) == (FULL, 1, 23)
    assert check_group(be, [s0, s1], [[(1, 8)], [(9, 12), (14, 31)]], max_size=3000) == (MISSING, 1, 31)

    # TRUNCATED: a selected record pointing past its file; the same record unselected is harmless
    recs = [R(1 + j, 1, p) for j, p in enumerate(rnd_payloads(rng, 10, 80))]
    recs[6]["ln"] = 5000
    t = make_source(recs)
    assert check_group(be, [s0, t], [[(1, 8)], [(1, 10)]]) == (TRUNCATED, 1, 7)
    assert isinstance(check_group(be, [s0, t], [[(1, 8)], [(1, 6), (8, 10)]]), bytes)
    recs[6]["ln"], recs[6]["off"] = None, (1 << 63)
    assert check_group(be, [make_source(recs)], [[(5, 9)]]) == (TRUNCATED, 0, 7)

    # SPACE: one byte short; file_bytes is still reported and nothing behind out_bytes is written
    want = ref_compact(*group)
    sources, buf, live = pack_group(*group)
    res, region = device_compact(be, sources, buf, live, out_bytes=len(want) - 1)
    assert (int(res["status"]), int(res["file_bytes"])) == (SPACE, len(want))
    res, region = device_compact(be, sources, buf, live, out_bytes=len(want))
    assert int(res["status"]) == OK and region.tobytes() == want
    out = np.full(len(want) - 1, 0xEE, dtype=np.uint8)
    res, image = be.eng.segment_compact(sources, buf, live, out=out)
    assert (int(res["status"]), int(res["file_bytes"])) == (SPACE, len(want)) and image is None and np.all(out == 0xEE)

    # CRC: a flipped byte in the third selected entry and one later; without the flag the flipped byte is copied
    pay = rnd_payloads(rng, 20, 400)
    pay[2], pay[4], pay[12] = pay[2] + b"x" * 40, pay[4] + b"y", pay[12] + b"z" * 17
    c = make_source([R(1 + j, 1, p) for j, p in enumerate(pay)])
    parsed = ref_parse(c)
    flipped = bytearray(c)
    for idx in (5, 13):                                     # live = 1, 3, 5, ...: index 5 is the third selected entry
        flipped[parsed[idx][1] + parsed[idx][2] // 2] ^= 0x01
    live_c = [(i, i) for i in range(1, 21, 2)]
    assert check_group(be, [s0, bytes(flipped)], [[], live_c], flags=VERIFY) == (CRC, 1, 5)
    assert isinstance(check_group(be, [s0, bytes(flipped)], [[], live_c], flags=0), bytes)
    assert isinstance(check_group(be, [s0, c], [[], live_c], flags=VERIFY), bytes)
    flipped[parsed[3][1]] ^= 0x80                           # damage in an entry that is not copied is not looked at
    assert isinstance(check_group(be, [bytes(flipped)], [[(6, 11)]], flags=VERIFY), bytes)

    # BAD_SOURCE on the device form, RGB_E_INVAL on the host-buffer form (inside check_group)
    for broken in (b"RASX" + s1[4:], s1[:7], b"RASG\x00\x03" + s1[6:], b"RASG\x00\x00" + s1[6:]):
        assert check_group(be, [s0, broken, b"RAS"], [[(1, 8)], [], []]) == (BAD_SOURCE, 1, 0)
        sources, buf, _ = pack_group([s0, broken], None)
        d_f, p_f, _ = be.dev(buf)
        d_i, p_i, b_i = be.dev(np.zeros(128, dtype=np.uint8))
        be.eng.segment_info_device(sources, p_f, len(buf), None, p_i)
        rows = be.get(d_i)[b_i:b_i + 128].copy().view(abi.SEG_INFO_DTYPE)
        assert [int(x) for x in rows["status"]] == [OK, BAD_SOURCE] and int(rows["version"][1]) == 0
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.segment_info(sources, buf, None)
        assert e.value.code == E_INVAL


PAY = 100                       # payload bytes of every record of the precedence cases: `pre` of place p is 100 p


def precedence_group(sources, full=None, bad_crc=None, broken=None):
    """A group whose faults fall on chosen PLACES of the copy order.  sources: per source (places, missing, trunc) --
    `places` records are selected; `missing`: the live index of that rank is absent from the file, so the record of the
    next rank takes its place; `trunc`: the record at that place points outside the file.  full = (source, place): the
    first place with more than max_size payload bytes in front of it.  bad_crc = (source, place): a stored Crc that
    does not match.  broken = source: its file header is damaged, which info/2 of every file meets before anything is
    copied, so it wins over every fault of any source.  -> (files, lives, max_size, (status, source, index) worked out
    from the places alone: the earliest
    place in copy order, MISSING before TRUNCATED before FULL at one place)."""
    files, lives, found, front = [], [], [], 0
    for s, (places, missing, trunc) in enumerate(sources):
        base = 1000 * s
        n_live = places + (missing is not None)
        idxs = [base + i for i in range(1, n_live + 1) if missing is None or i != missing + 1]
        recs = [R(i, 1 + s, bytes([i % 251]) * PAY) for i in idxs]
        if trunc is not None:
            recs[trunc]["off"] = 1 << 40
        if bad_crc is not None and bad_crc[0] == s:
            recs[bad_crc[1]]["crc"] = 0x1234567
        files.append(make_source(recs))
        lives.append([(base + 1, base + n_live)])
        here = []
        if missing is not None:
            here.append((missing, 0, MISSING, base + missing + 1))
        if trunc is not None:
            here.append((trunc, 1, TRUNCATED, idxs[trunc]))
        if full is not None and full[0] == s:
            here.append((full[1], 2, FULL, idxs[full[1]]))
            max_size = front + PAY * full[1] - 1
            assert max_size >= 0, "nothing can be full at the very first place of a group"
        if here:
            found.append((s,) + min(here))
        front += PAY * places
    expect = (found[0][3], found[0][0], found[0][4]) if found else None
    if broken is not None:
        files[broken] = b"RASX" + files[broken][4:]
        expect = (BAD_SOURCE, broken, 0)
    return files, lives, (max_size if full is not None else MAX_SIZE), expect


def check_status_precedence(be, width, flags):
    """MISSING, TRUNCATED and FULL on ONE place of the copy order, and one place or one source apart: the reference
    meets the missing key first (is_map_key), then reads the payload, then append_raw asks is_full
    (src/ra_log_segment.erl:819-908), so at one place MISSING wins over TRUNCATED over FULL and otherwise the
    earlier place wins whatever its kind; a stored Crc that does not match never wins (it is looked at last).
    Referee: ref_compact, which walks in that order; the expectation worked out from the places has to agree with it."""
    def run(sources, full=None, bad_crc=None, broken=None, host_form=False, what=""):
        files, lives, max_size, expect = precedence_group(sources, full, bad_crc, broken)
        files = pad_to_width(files, sum(len(_expand(l)) for l in lives), width)
        got = check_group(be, files, lives, max_size=max_size, flags=flags, host_form=host_form, what=what)
        assert got == expect, f"{what}: the referee says {got}, the places say {expect}"

    front = (1, None, None)                                  # a clean source of one entry: bytes in front of place 0
    # first, middle and last place of a short selection; both sides of the resolve pass's chunk edge, in the middle of a
    # selection and as its last place
    for k, places in ((0, 1), (0, 9), (4, 9), (8, 9), (255, 260), (256, 260), (257, 260), (255, 256), (256, 257)):
        tag = f"place {k} of {places}"
        pre, s = ([front], 1) if k == 0 else ([], 0)         # (FULL at place 0 needs bytes of an earlier source)
        run([(places, k, k)], what=f"(a) {tag}", host_form=k == 4)
        run(pre + [(places, k, None)], full=(s, k), what=f"(b) {tag}", host_form=k == 4)
        run(pre + [(places, None, k)], full=(s, k), what=f"(c) {tag}", host_form=k == 4)
        run(pre + [(places, k, k)], full=(s, k), what=f"(d) {tag}", host_form=k == 4)
        # (e) one place apart, both orders: the earlier place wins whatever its kind
        for lo, hi in ((k - 1, k), (k, k + 1)):
            if lo < 0 or hi >= places:
                continue
            for first, second in (("M", "T"), ("T", "M"), ("M", "F"), ("F", "M"), ("T", "F"), ("F", "T")):
                at = {first: lo, second: hi}
                if at.get("F") == 0:
                    continue                                 # (covered by (b)-(d) at k = 0, behind `front`)
                run([(places, at.get("M"), at.get("T"))], full=(0, at["F"]) if "F" in at else None,
                    what=f"(e) {first} at {lo}, {second} at {hi} of {places}")
    # (f) the offending place in the second source; a lower-precedence fault one source later; a higher one earlier
    clean, k = (40, None, None), 17
    for name, spec, full in (("a", (60, k, k), None), ("b", (60, k, None), (1, k)), ("c", (60, None, k), (1, k)),
                             ("d", (60, k, k), (1, k))):
        run([clean, spec], full=full, what=f"(f) ({name}) in the second source", host_form=True)
    run([clean, (60, None, k), (30, 0, None)], what="(f) TRUNCATED, MISSING one source later")
    run([clean, (60, k, None), (30, None, 0)], what="(f) MISSING, TRUNCATED one source later")
    run([clean, (60, None, k), (30, 0, 0)], full=(1, k), what="(f) TRUNCATED + FULL, everything one source later")
    run([(40, 39, None), (60, None, None)], full=(1, k), what="(f) FULL, MISSING at the last rank one source earlier")
    run([(40, None, 39), (60, k, None)], what="(f) MISSING, TRUNCATED at the last place one source earlier")
    run([(40, None, 0), (60, k, k)], full=(1, k), what="(f) all three, TRUNCATED one source earlier")
    # BAD_SOURCE first: a damaged header in a LATER source wins over MISSING, TRUNCATED and FULL of an earlier one, and
    # over a Crc mismatch; the first damaged file is named
    for name, spec, full in (("a", (60, k, k), None), ("b", (60, k, None), (0, k)), ("c", (60, None, k), (0, k)),
                             ("d", (60, k, k), (0, k))):
        run([spec, clean], full=full, broken=1, what=f"BAD_SOURCE behind ({name})", host_form=True)
    run([clean, (60, None, 0), clean], broken=2, what="BAD_SOURCE two sources behind TRUNCATED at place 0")
    run([(60, None, None), clean, clean], bad_crc=(0, 3), broken=1, what="BAD_SOURCE behind a Crc mismatch")
    run([(60, k, None), clean, clean, clean], broken=3, what="BAD_SOURCE in the last source, MISSING in the first")
    files, lives, _, _ = precedence_group([(60, k, k), clean, clean])
    files = pad_to_width(files, sum(len(_expand(l)) for l in lives), width)
    files[1], files[2] = files[1][:7], b"RASG\x00\x03" + files[2][6:]
    got = check_group(be, files, lives, flags=flags, host_form=False, what="two damaged files: the first is named")
    assert got == (BAD_SOURCE, 1, 0)
    # (g) a stored Crc mismatch at an earlier place: with VERIFY it is still not CRC (and without, not looked at)
    for name, spec, full in (("a", (60, k, k), None), ("b", (60, k, None), (0, k)), ("c", (60, None, k), (0, k)),
                             ("d", (60, k, k), (0, k))):
        run([spec], full=full, bad_crc=(0, k - 1), what=f"(g) ({name}) behind a Crc mismatch", host_form=True)
    # ... and the mismatch alone is CRC with the flag, nothing without
    files, lives, _, _ = precedence_group([(60, None, None)], bad_crc=(0, k - 1))
    files = pad_to_width(files, 60, width)
    got = check_group(be, files, lives, flags=flags, what="(g) the mismatch alone")
    assert got == (CRC, 0, k) if flags & VERIFY else isinstance(got, bytes)


SPREAD_RECORDS = 600            # three steps of the resolve pass; 19 to 150 workgroups of the copy, by the lane-group width
SPREAD_PLACES = (330, 200, 40)  # 40 and 200: one step of the resolve pass, two wavefronts; 40 and 330: 290 places apart


def check_spread_faults(be, width, flags):
    """The SAME fault at three places of one source's copy order, far apart: the answer is the first in copy order, and
    the kernels find it as a minimum over atomics (s_miss_k, s_trunc_k, hdr->crc_fail, s_first_zero) that reach their
    word in whatever order lanes and workgroups run.  Places 40 and 200 meet in one step of the resolve pass, on
    different wavefronts; 40 and 330 are 290 places apart, in different workgroups of the copy.  Referee: ref_compact."""
    n, first = SPREAD_RECORDS, min(SPREAD_PLACES)
    verify = bool(flags & VERIFY)

    def records(skip=()):
        return [R(i, 2, bytes([i % 251]) * 20) for i in range(1, n + 1 + len(skip)) if i - 1 not in skip]

    def run(files, lives, expect, what):
        files = pad_to_width(files, sum(len(_expand(l)) for l in lives), width)
        got = check_group(be, files, lives, flags=flags, host_form=False, what=what)
        assert (got == expect) if expect is not None else isinstance(got, bytes), f"{what}: the referee says {got}, want {expect}"

    recs = records()
    for p in SPREAD_PLACES:
        recs[p]["crc"] = 0x1234567
    run([make_source(recs)], [[(1, n)]], (CRC, 0, first + 1) if verify else None, "three Crc mismatches")
    recs = records()
    for p in SPREAD_PLACES:
        recs[p]["off"] = 1 << 40
    run([make_source(recs)], [[(1, n)]], (TRUNCATED, 0, first + 1), "three truncated records")
    # three live indexes that the file does not have: every selected record behind the first of them is off its rank
    run([make_source(records(skip=SPREAD_PLACES))], [[(1, n + 3)]], (MISSING, 0, first + 1), "three missing indexes")
    # one of each, the later place the higher-ranking kind
    recs = records(skip=(330,))
    recs[200]["off"] = 1 << 40
    recs[40]["crc"] = 0x1234567
    run([make_source(recs)], [[(1, n + 1)]], (TRUNCATED, 0, 201), "Crc at 40, TRUNCATED at 200, MISSING at 330")
    # the fault of the LOWER-numbered source lies later in its copy order than the fault of the next source
    a, b = records(), [R(1000 + i, 3, bytes([i]) * 20) for i in range(60)]
    a[330]["crc"] = b[5]["crc"] = 0x1234567
    run([make_source(a), make_source(b)], [[(1, n)], [(1000, 1059)]], (CRC, 0, 331) if verify else None,
        "a mismatch at place 330 of source 0 and at place 5 of source 1")
    # the walk ends at the first all-zero record: 40 records and 300 unused ones, 216 of them in the first step
    short = make_source(records()[:first], max_count=first + 300)
    check_info(be, [short], [[(1, first)]], "300 all-zero records behind 40")
    run([short], [[(1, first)]], None, "300 all-zero records behind 40")


def malformed_descriptors():
    """(name, sources, live pairs, files_bytes, flags) -- each is RGB_E_INVAL"""
    def src(*rows):
        s = np.zeros(len(rows), dtype=abi.SEG_SOURCE_DTYPE)
        for i, (off, nb, lf, ln) in enumerate(rows):
            s["offset"][i], s["n_bytes"][i], s["live_first"][i], s["live_n"][i] = off, nb, lf, ln
        return s
    U = (1 << 64) - 1
    return [("not ascending", src((0, 100, 0, 2)), [(10, 12), (5, 6)], 100, 0),
            ("overlapping", src((0, 100, 0, 2)), [(10, 12), (12, 14)], 100, 0),
            ("adjacent", src((0, 100, 0, 2)), [(10, 12), (13, 14)], 100, 0),
            ("first > last", src((0, 100, 0, 1)), [(9, 8)], 100, 0),
            ("adjacent across 2^64", src((0, 100, 0, 2)), [(1, U), (0, 3)], 100, 0),
            ("slice outside the list", src((0, 100, 1, 2)), [(1, 2), (4, 5)], 100, 0),
            ("slice start outside the list", src((0, 100, 3, 0)), [(1, 2), (4, 5)], 100, 0),
            ("slice wraps", src((0, 100, 0xFFFFFFFF, 2)), [(1, 2), (4, 5)], 100, 0),
            ("source outside the files buffer", src((0, 50, 0, 1), (60, 41, 1, 1)), [(1, 2), (4, 5)], 100, 0),
            ("source offset wraps", src((U - 3, 8, 0, 1)), [(1, 2)], 100, 0),
            ("MaxCount 65536", src((0, 100, 0, 1)), [(1, 65536)], 100, 0),
            ("MaxCount 65536 over two sources", src((0, 100, 0, 1), (0, 100, 1, 1)), [(1, 65535), (3, 3)], 100, 0),
            ("a range of 2^64", src((0, 100, 0, 1)), [(0, U)], 100, 0),
            ("too many sources", np.zeros(abi.SEG_COMPACT_MAX_SOURCES + 1, dtype=abi.SEG_SOURCE_DTYPE), [], 100, 0),
            ("unknown flags", src((0, 100, 0, 1)), [(1, 2)], 100, 2)]


def check_argument_errors(be):
    buf = np.frombuffer(make_source([R(1, 1, b"abc"), R(2, 1, b"defg")], tail=60)[:100], dtype=np.uint8).copy()
    assert len(buf) == 100
    for name, sources, pairs, files_bytes, flags in malformed_descriptors():
        live = np.array(pairs, dtype=np.uint64).reshape(-1, 2)
        if not flags:
            with pytest.raises(be.engine.RgbError) as e:
                be.engine.segment_compact_bound(sources, live, files_bytes)
            assert e.value.code == E_INVAL, name
        out = np.full(400, 0xEE, dtype=np.uint8)
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.segment_compact(sources, buf, live, MAX_SIZE, flags, out=out)
        assert e.value.code == E_INVAL and np.all(out == 0xEE), name
        d_f, p_f, _ = be.dev(buf)
        d_o, p_o, b_o = be.dev(np.full(432, 0xEE, dtype=np.uint8))
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.segment_compact_device(sources, p_f, files_bytes, live, p_o, 400, p_o + 400, MAX_SIZE, flags)
        assert e.value.code == E_INVAL, name
        assert np.all(be.get(d_o)[b_o:b_o + 432] == 0xEE), f"{name}: refused, but something was written"
        if not flags and "MaxCount" not in name and "2^64" not in name:       # info counts nothing: any range is fine
            with pytest.raises(be.engine.RgbError) as e:
                be.eng.segment_info_device(sources, p_f, files_bytes, live, p_o)
            assert e.value.code == E_INVAL, name
            assert np.all(be.get(d_o)[b_o:b_o + 432] == 0xEE), name
    # the limits themselves are legal
    sources = np.zeros(abi.SEG_COMPACT_MAX_SOURCES, dtype=abi.SEG_SOURCE_DTYPE)
    sources["n_bytes"] = 8
    assert be.engine.segment_compact_bound(sources, None, 100) == (8 + 8 * abi.SEG_COMPACT_MAX_SOURCES, 0)
    one = np.zeros(1, dtype=abi.SEG_SOURCE_DTYPE); one["n_bytes"], one["live_n"] = 100, 1
    assert be.engine.segment_compact_bound(one, [(1, 65535)], 100) == (8 + 32 * 65535 + 100, 65535)


# ------------------------------------------------------------------------------------------ CPU (emulation)

def test_abi_mirror():
    hdr = open(os.path.join(ROOT, "include", "ra_gpu_wal.h")).read()
    flat = " ".join(hdr.split())
    for name, val in (("RGB_SEG_COMPACT_OK", OK), ("RGB_SEG_COMPACT_MISSING", MISSING), ("RGB_SEG_COMPACT_FULL", FULL),
                      ("RGB_SEG_COMPACT_TRUNCATED", TRUNCATED), ("RGB_SEG_COMPACT_SPACE", SPACE),
                      ("RGB_SEG_COMPACT_CRC", CRC), ("RGB_SEG_COMPACT_BAD_SOURCE", BAD_SOURCE),
                      ("RGB_SEG_COMPACT_VERIFY", abi.SEG_COMPACT_VERIFY),
                      ("RGB_SEG_COMPACT_MAX_SOURCES", abi.SEG_COMPACT_MAX_SOURCES),
                      ("RGB_SEG_MAX_SIZE_DEFAULT", abi.SEG_MAX_SIZE_B)):
        assert int(flat.split(f"#define {name} ")[1].split()[0].rstrip("ul")) == val, name
    assert abi.SEG_COMPACT_MAX_SOURCES >= 64 and (OK, BAD_SOURCE) == (abi.SEG_COMPACT_OK, abi.SEG_COMPACT_BAD_SOURCE)
    assert "#define RGB_ABI_VERSION 10" in " ".join(open(os.path.join(ROOT, "include", "ra_gpu_batch.h")).read().split())
    assert abi.SEG_SOURCE_DTYPE.fields["live_first"][1] == 16 and abi.SEG_INFO_DTYPE.fields["num_entries"][1] == 40
    assert abi.SEG_COMPACT_RESULT_DTYPE.fields["index"][1] == 16 and abi.SEG_COMPACT_RESULT_DTYPE.fields["source"][1] == 24


def test_referee_on_a_worked_example():
    """The referee itself, on a case small enough to do by hand (the trim rule of :1063-1069)."""
    f = make_source([R(1, 1, b"a"), R(2, 1, b"bb"), R(3, 1, b"ccc"), R(2, 2, b"dddd"), R(2, 3, b"e"), R(5, 3, b"ff")])
    start = 8 + 32 * 6
    assert ref_parse(f) == {1: (1, start, 1, zlib.crc32(b"a")), 2: (3, start + 10, 1, zlib.crc32(b"e")),
                            5: (3, start + 11, 2, zlib.crc32(b"ff"))}
    info = ref_info(f, [(2, 3)])
    assert (info["num_entries"], info["size"], info["range"], info["indexes"]) == (6, start + 13, (1, 5), [1, 2, 5])
    assert info["live_size"] == 2 + 3 + 4 + 1               # every walked record whose Idx is live, trimmed ones too
    assert ref_compact([f], [[(1, 3)]]) == (MISSING, 0, 3)
    image = ref_compact([f], [[(1, 2), (5, 5)]])
    assert image == python_segment([(1, 1), (2, 3), (5, 3)], [b"a", b"e", b"ff"], 3)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_emu_effective_scan(emu, n):
    check_effective_scan(emu, n)


def test_emu_versions_and_walk_ends(emu):
    check_versions_and_walk_ends(emu)


def test_emu_live_slices(emu):
    check_live_slices(emu)


def test_emu_same_index_in_two_sources(emu):
    check_same_index_in_two_sources(emu)


def test_emu_stored_crc_zero(emu):
    check_stored_crc_zero(emu)


@pytest.mark.parametrize("width", [8, 16, 64])
def test_emu_payload_shapes(emu, width):
    check_payload_shapes(emu, width)


@pytest.mark.parametrize("flags", [0, VERIFY], ids=["plain", "verify"])
@pytest.mark.parametrize("width", [8, 16, 64])
def test_emu_every_phase(emu, width, flags):
    check_every_phase(emu, width, flags)


def test_emu_statuses(emu):
    check_statuses(emu)


@pytest.mark.parametrize("flags", [0, VERIFY], ids=["plain", "verify"])
@pytest.mark.parametrize("width", [8, 16, 64])
def test_emu_status_precedence(emu, width, flags):
    check_status_precedence(emu, width, flags)


@pytest.mark.parametrize("flags", [0, VERIFY], ids=["plain", "verify"])
@pytest.mark.parametrize("width", [8, 16, 64])
def test_emu_spread_faults(emu, width, flags):
    check_spread_faults(emu, width, flags)


@pytest.mark.parametrize("sched", PERMUTED_SCHEDULES)
def test_emu_under_permuted_schedules(emu, sched):
    """The emulation's own order is workgroups 0, 1, 2, ... and lanes 0 .. 255, so every "first in order" that the
    kernels take as a minimum over atomics also arrives first.  The checks whose answers are such minima, sums and bit
    sets once more with workgroups and lanes reversed and permuted (tests/emu_schedule.py); the referee stays
    ref_compact / ref_info."""
    with schedule(emu.engine, sched):
        for width in (8, 16, 64):
            for flags in (0, VERIFY):
                check_status_precedence(emu, width, flags)
                check_spread_faults(emu, width, flags)
        check_effective_scan(emu, 257)
        check_effective_scan(emu, 1000)
        check_same_index_in_two_sources(emu)
        check_statuses(emu)


def test_emu_argument_errors(emu):
    check_argument_errors(emu)


def test_emu_back_to_back_calls(emu):
    check_back_to_back_calls(emu)


def test_compact_descriptors_under_sanitizers(tmp_path):
    """rgb_segment_compact_bound -- the host-side validation of every compact call, in the host-only unit
    rgb_segment_host.cpp -- compiled with AddressSanitizer + UBSan into a stand-alone program and run over the malformed
    descriptors of check_argument_errors and some good ones, each array in an exactly-sized heap block."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "segment_compact_harness"
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-o", str(exe),
           os.path.join(ROOT, "tests", "native", "segment_compact_harness.cpp"),
           os.path.join(ROOT, "ra_amd", "csrc", "rgb_segment_host.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert built.returncode == 0, built.stderr
    cases = [(s, l, fb, E_INVAL, 0, 0) for _, s, l, fb, flags in malformed_descriptors() if not flags]
    good = np.zeros(3, dtype=abi.SEG_SOURCE_DTYPE)
    good["offset"], good["n_bytes"], good["live_first"], good["live_n"] = (0, 40, 90), (40, 50, 10), (0, 2, 2), (2, 0, 1)
    cases.append((good, [(1, 5), (7, 7), (3, 65000)], 100, 0, 8 + 32 * 65004 + 100, 65004))
    cases.append((good[:0], [], 0, 0, 8, 0))
    files = []
    for k, (s, l, fb, _, _, _) in enumerate(cases):
        path = tmp_path / f"d{k}.bin"
        path.write_bytes(struct.pack("<IIQ", len(s), len(l), fb) + s.tobytes() +
                         np.array(l, dtype=np.uint64).reshape(-1, 2).tobytes())
        files.append(str(path))
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in run.stdout.splitlines()]
    assert got == [c[3:] for c in cases]


def test_compact_kernels_use_no_scratch():
    """hipcc's resource remarks for gfx950 (no GPU needed), as tests/test_kernel_resources.py reads them: the kernels
    of the three passes without scratch or spills; the copy without VERIFY uses no LDS (no table lookups at all), the
    one with VERIFY the 20 KiB of the CRC kernels."""
    from test_kernel_resources import segment_usage
    usage = segment_usage()
    names = [k for k in usage if "rgb_compact_" in k]
    assert len(names) == 9, names                       # resolve, place, finish, 3 widths x {verify, plain}
    for k in names:
        u = usage[k]
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, f"{k}: {u}"
        assert u["Occupancy"] >= 7 and u["LDS Size"] <= 20 * 1024 + 64, f"{k}: {u}"
        if "copy_kernel" in k and "ELb0E" in k:             # <GROUP, VERIFY = false>
            assert u["LDS Size"] <= 64, f"{k}: the plain copy must not hold the CRC tables"


# ------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_gpu_effective_scan(gpu, n):
    check_effective_scan(gpu, n)


@pytest.mark.gpu
def test_gpu_scan_width(gpu):
    """GPU only: the emulation runs the 256 chunks of this index as 256 fibers x ~40 barrier intervals each and the
    copy as 2048 blocks of fibers, which takes it far beyond the few seconds a test may cost."""
    check_scan_width(gpu)


@pytest.mark.gpu
def test_gpu_versions_and_walk_ends(gpu):
    check_versions_and_walk_ends(gpu)


@pytest.mark.gpu
def test_gpu_live_slices(gpu):
    check_live_slices(gpu)


@pytest.mark.gpu
def test_gpu_same_index_in_two_sources(gpu):
    check_same_index_in_two_sources(gpu)


@pytest.mark.gpu
def test_gpu_stored_crc_zero(gpu):
    check_stored_crc_zero(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [8, 16, 64])
def test_gpu_payload_shapes(gpu, width):
    check_payload_shapes(gpu, width)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, VERIFY], ids=["plain", "verify"])
@pytest.mark.parametrize("width", [8, 16, 64])
def test_gpu_every_phase(gpu, width, flags):
    check_every_phase(gpu, width, flags)


@pytest.mark.gpu
def test_gpu_statuses(gpu):
    check_statuses(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, VERIFY], ids=["plain", "verify"])
@pytest.mark.parametrize("width", [8, 16, 64])
def test_gpu_status_precedence(gpu, width, flags):
    check_status_precedence(gpu, width, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, VERIFY], ids=["plain", "verify"])
@pytest.mark.parametrize("width", [8, 16, 64])
def test_gpu_spread_faults(gpu, width, flags):
    check_spread_faults(gpu, width, flags)


@pytest.mark.gpu
def test_gpu_argument_errors(gpu):
    check_argument_errors(gpu)


@pytest.mark.gpu
def test_gpu_back_to_back_calls(gpu):
    check_back_to_back_calls(gpu)
