"""Batched segment reads on the device: rgb_segment_read* (include/ra_gpu_wal.h, "reading entries back";
ra_amd/csrc/rgb_segment.hip, rgb_segment_host.cpp).

Referee: ref_read, pure Python, written sequentially from the reference source with a dict --
  the map        parse_index_data_loop   src/ra_log_segment.erl:1057-1075 (ref_parse of tests/test_segment_compact.py)
  one lookup     read_sparse/4, fold0/8, term_query/2   :375-598, :661-689, :652-659: maps:get per requested index, in
                 the caller's order; a key that is not there is exit({missing_key, Idx}) / not_found
  the checksum   validate_checksum/2     :1245-1248 with zlib.crc32 (a stored Crc of 0 is not checked)
-- plus what include/ra_gpu_wal.h defines and the reference does not: a found record whose payload lies outside its file
is TRUNCATED (DataOffset > n_bytes or Length > n_bytes - DataOffset), a MISSING or TRUNCATED row is
{requested index, 0, RGB_UNDEF, 0, 0} and takes no bytes, the per-source result names the first bad row in request
order (MISSING and TRUNCATED before CRC), a bad header makes every row of the slice a MISSING row, and out_bytes below
the bytes needed is SPACE: rows and results as they would be, no CRC status, `out` untouched.  The library finds a
request by binary search in a table of the effective records; the referee deliberately has neither.

Rows, results, the total and `out` are compared byte for byte; rows and `out` sit between guard bytes.

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
from test_segment_compact import R, make_source, pad_to_width, ref_parse, scan_patterns, source_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL = -1
OK, MISSING, TRUNCATED, CRC, BAD_SOURCE, SPACE = range(6)
VERIFY, NO_DATA = abi.SEG_READ_VERIFY, abi.SEG_READ_NO_DATA
UNDEF = (1 << 64) - 1
STEP = 256                     # rgb_segment.hip: records, requests and sources per step of a workgroup (THREADS)
GUARD = 64
ROW = "<QQQII"                 # rgb_seg_entry
POISON = 0xEE


# ------------------------------------------------------------------------------------------ referee

def _bad_header(f: bytes) -> bool:
    return len(f) < 8 or f[:4] != b"RASG" or struct.unpack(">H", f[4:6])[0] not in (1, 2)


def ref_read(files, sources, req, flags=0, out_bytes=None):
    """files[s]: the bytes of source s; sources: the descriptors (offset for NO_DATA, the slices).  out_bytes None: room
    enough.  -> dict(rows, results, total, out: bytes as the library leaves them, a never-written row being POISON;
    statuses: [(status, n_read, index)], needed)."""
    verify, no_data = bool(flags & VERIFY), bool(flags & NO_DATA)
    rows = bytearray([POISON]) * (32 * len(req))
    out, per_source = bytearray(), []
    for s, f in enumerate(files):
        first, n = int(sources["req_first"][s]), int(sources["req_n"][s])
        index = None if _bad_header(f) else ref_parse(f)
        bad, mismatch, data_bytes = None, None, 0
        for k in range(n):
            idx = int(req[first + k])
            kind = OK
            if index is None or idx not in index:
                kind = MISSING
            else:
                term, pos, length, crc = index[idx]
                if pos > len(f) or length > len(f) - pos:
                    kind = TRUNCATED
            if kind != OK:
                row = (idx, 0, UNDEF, 0, 0)
                if bad is None:
                    bad = (kind, k, idx)
            else:
                data = f[pos:pos + length]
                if no_data:
                    row = (idx, term, int(sources["offset"][s]) + pos, length, crc)
                else:
                    row = (idx, term, len(out), length, crc)
                    out += data
                    data_bytes += length
                if verify and crc != 0 and zlib.crc32(data) != crc and mismatch is None:
                    mismatch = (CRC, k, idx)
            rows[32 * (first + k):32 * (first + k + 1)] = struct.pack(ROW, *row)
        if index is None:
            bad = (BAD_SOURCE, 0, 0)
        per_source.append((bad, mismatch, n, data_bytes))
    needed = len(out)
    space = out_bytes is not None and out_bytes < needed
    statuses = []
    for bad, mismatch, n, data_bytes in per_source:
        st = bad or (mismatch if not space else None) or (OK, n, 0)
        statuses.append(st)
    results = b"".join(struct.pack("<IIQQQ", st[0], st[1], st[2], p[3], 0) for st, p in zip(statuses, per_source))
    total = struct.pack("<IIQ", SPACE if space else OK, sum(1 for st in statuses if st[0] != OK), needed)
    return dict(rows=bytes(rows), results=results, total=total, out=b"" if space else bytes(out), statuses=statuses,
                needed=needed, space=space)


def test_referee_on_a_worked_example():
    """Three records, the third steps backwards over the second: 7 is trimmed, 5 is overwritten by the later record."""
    f = make_source([R(5, 1, b"five"), R(7, 1, b"seven"), R(5, 2, b"FIVE!"), R(9, 2, b"")], max_count=6)
    assert ref_parse(f) == {5: (2, 8 + 6 * 32 + 9, 5, zlib.crc32(b"FIVE!")), 9: (2, 8 + 6 * 32 + 14, 0, 0)}
    src = np.zeros(1, dtype=abi.SEG_READ_SOURCE_DTYPE)
    src["n_bytes"], src["req_n"] = len(f), 4
    want = ref_read([f], src, [9, 5, 7, 5])
    assert want["out"] == b"FIVE!FIVE!" and want["statuses"] == [(MISSING, 2, 7)]
    rows = [struct.unpack(ROW, want["rows"][32 * k:32 * k + 32]) for k in range(4)]
    assert rows == [(9, 2, 0, 0, 0), (5, 2, 0, 5, zlib.crc32(b"FIVE!")), (7, 0, UNDEF, 0, 0), (5, 2, 5, 5, zlib.crc32(b"FIVE!"))]
    assert want["total"] == struct.pack("<IIQ", OK, 1, 10)
    assert ref_read([f], src, [9, 5, 7, 5], 0, 9)["total"] == struct.pack("<IIQ", SPACE, 1, 10)


# ------------------------------------------------------------------------------------------ building inputs

def pack_read(files, slices, gaps=None, alias=None):
    """-> (descriptors, the files buffer).  alias {s: t}: source s names the very bytes of source t."""
    buf = bytearray()
    sources = np.zeros(len(files), dtype=abi.SEG_READ_SOURCE_DTYPE)
    for s, f in enumerate(files):
        if alias and s in alias:
            sources["offset"][s], sources["n_bytes"][s] = sources["offset"][alias[s]], sources["n_bytes"][alias[s]]
        else:
            buf += b"\xa5" * (gaps[s] if gaps else 3 * (s % 7) + 1)
            sources["offset"][s], sources["n_bytes"][s] = len(buf), len(f)
            buf += f
        sources["req_first"][s], sources["req_n"][s] = slices[s]
    buf += b"\xa5" * 5
    return sources, np.frombuffer(bytes(buf), dtype=np.uint8).copy()


def slices_of(reqs, holes=None):
    """reqs[s]: the requests of source s -> (slices, the flat list); holes[s] requests that no slice names in front of
    slice s (and holes[len(reqs)] behind the last)."""
    flat, slices = [], []
    for s, r in enumerate(reqs):
        flat += [77] * (holes[s] if holes else 0)
        slices.append((len(flat), len(r)))
        flat += list(r)
    flat += [77] * (holes[len(reqs)] if holes else 0)
    return slices, np.array(flat, dtype=np.uint64)


def guarded(n, fill=POISON):
    return np.concatenate([np.full(GUARD, 0xC3, dtype=np.uint8), np.full(n, fill, dtype=np.uint8),
                           np.full(GUARD, 0xC3, dtype=np.uint8)])


def inside(got, base, n, what):
    assert np.all(got[:base] == 0) and np.all(got[base + n + 2 * GUARD:] == 0), f"wrote outside the buffer of {what}"
    assert np.all(got[base:base + GUARD] == 0xC3), f"wrote in front of {what}"
    assert np.all(got[base + GUARD + n:base + n + 2 * GUARD] == 0xC3), f"wrote behind {what}"
    return got[base + GUARD:base + GUARD + n].tobytes()


# ------------------------------------------------------------------------------------------ calling the library

def device_read(be, sources, buf, req, flags=0, out_bytes=0, src_phase=0, dst_phase=0, null_out=False):
    """-> (rows, results, total, out) as bytes, through rgb_segment_read_device; everything is poisoned first and the
    guard bytes around rows and out are checked."""
    n_req, n_src = len(req), len(sources)
    d_f, p_f, _ = be.dev(buf, src_phase)
    d_w, p_w, b_w = be.dev(guarded(32 * n_req))
    d_o, p_o, b_o = be.dev(guarded(out_bytes), dst_phase)
    d_r, p_r, b_r = be.dev(np.full(32 * n_src, 0x77, dtype=np.uint8))
    d_t, p_t, b_t = be.dev(np.full(16, 0x77, dtype=np.uint8))
    be.eng.segment_read_device(sources, p_f, len(buf), req, p_w + GUARD, 0 if null_out else p_o + GUARD, out_bytes, p_r, p_t,
                               flags)
    rows = inside(be.get(d_w), b_w, 32 * n_req, "d_rows")
    out = inside(be.get(d_o), b_o, out_bytes, "d_out")
    del d_f
    return rows, be.get(d_r)[b_r:b_r + 32 * n_src].tobytes(), be.get(d_t)[b_t:b_t + 16].tobytes(), out


def same(got, want, what):
    diff = first_diff(got, want)
    assert diff is None, f"{what}: {diff}"


def check_read(be, files, slices, req, flags=0, space=False, src_phase=0, dst_phase=0, alias=None, gaps=None,
               host_form=True, slack=24, what=""):
    """Both forms against the referee, byte for byte.  space: out_bytes = needed - 1.  -> the referee's answer."""
    req = np.asarray(req, dtype=np.uint64)
    sources, buf = pack_read(files, slices, gaps, alias)
    real = [files[alias[s]] if alias and s in alias else f for s, f in enumerate(files)]
    needed = ref_read(real, sources, req, flags)["needed"]
    if space:
        assert needed > 0, f"{what}: nothing to be short of"
    out_bytes = needed - 1 if space else needed + slack
    want = ref_read(real, sources, req, flags, out_bytes)
    assert want["space"] == space
    want_out = want["out"] + bytes([POISON]) * (out_bytes - len(want["out"]))
    rows, results, total, out = device_read(be, sources, buf, req, flags, out_bytes, src_phase, dst_phase)
    same(total, want["total"], f"{what}: total")
    same(results, want["results"], f"{what}: results")
    same(rows, want["rows"], f"{what}: rows")
    same(out, want_out, f"{what}: out")
    if host_form:
        h_rows = np.full(32 * len(req), POISON, dtype=np.uint8).view(abi.SEG_ENTRY_DTYPE)
        h_out = np.full(out_bytes, POISON, dtype=np.uint8)
        tot, res, _, data = be.eng.segment_read(sources, buf, req, flags, rows=h_rows, out=h_out)
        same(tot.tobytes(), want["total"], f"{what}: host form, total")
        same(res.tobytes(), want["results"], f"{what}: host form, results")
        same(h_rows.tobytes(), want["rows"], f"{what}: host form, rows")
        same(h_out.tobytes(), want_out, f"{what}: host form, out")
        assert (data is None) == space
    return want


def kinds(want):
    return [st[0] for st in want["statuses"]]


# ------------------------------------------------------------------------------------------ the checks

SOURCE_SIZES = [0, 1, 255, 256, 257, 513]     # one either side of the resolve step, two steps and one


def check_source_sizes(be, n):
    """n records, MaxCount equal to and above n, both versions; every index asked in file order, one below and one
    above the range, and the Idx of an all-zero tail record; then the same file cut inside its index region."""
    rng = np.random.default_rng(700 + n)
    idxs = list(range(100, 100 + n))
    files = [source_of(rng, idxs, max_count=mc, version=v) for v in (2, 1) for mc in sorted({n, n + 3})]
    ask = idxs + [99, 100 + n, 0]
    slices, req = slices_of([ask] * len(files))
    for flags in (0, VERIFY, NO_DATA):
        want = check_read(be, files, slices, req, flags, what=f"n {n} flags {flags}")
        assert all(st == (MISSING, n, 99) for st in want["statuses"])
    if n >= 2:                                   # the file ends inside record n - 1: n - 1 records are walked, their payloads gone
        cut = [f[:8 + (32 if f[5] == 2 else 28) * (n - 1) + 5] for f in files]
        want = check_read(be, cut, slices, req, what=f"n {n}, cut inside the index region")
        assert all(st == (TRUNCATED, 0, 100) for st in want["statuses"])
        for f in cut:
            assert len(ref_parse(f)) == n - 1
        rows = [struct.unpack(ROW, want["rows"][32 * k:32 * k + 32]) for k in range(len(ask))]
        assert rows[n - 1] == (100 + n - 1, 0, UNDEF, 0, 0)                # the record the cut went through: MISSING


def check_index_shapes(be):
    """Backwards steps (one, several, across a step boundary of the resolve pass), an equal Idx repeated, a late record
    lower than everything: every Idx that occurs in the file is asked, trimmed ones included, and 0, and both sides of
    the range."""
    rng = np.random.default_rng(710)
    pats = [("one_backwards", [10, 11, 12, 13, 11, 12, 14]),
            ("several_backwards", [10, 11, 12, 9, 10, 11, 8, 20, 21, 19, 30]),
            ("equal_repeated", [10, 11, 11, 11, 12, 12, 13]),
            ("down_to_one_key", [10, 11, 12, 13, 1])]
    pats += scan_patterns(257, rng) + scan_patterns(513, rng)
    files, reqs, trimmed_asked = [], [], 0
    for _, seq in pats:
        f = source_of(rng, seq)
        files.append(f)
        ask = sorted(set(seq)) + [0, min(seq) - 1, max(seq) + 1]
        trimmed_asked += sum(1 for i in set(seq) if i not in ref_parse(f))
        reqs.append(ask)
    assert trimmed_asked > 500                          # the walks and the backwards steps do trim
    slices, req = slices_of(reqs)
    want = check_read(be, files, slices, req, what=", ".join(p[0] for p in pats))
    assert MISSING in kinds(want)
    # the later of two equal Idx wins: its term, its payload
    f = make_source([R(4, 1, b"old-old-old"), R(4, 2, b"new")])
    want = check_read(be, [f], [(0, 1)], [4], what="equal Idx")
    assert want["out"] == b"new" and struct.unpack(ROW, want["rows"])[1] == 2


def check_request_shapes(be):
    """One source of 700 records behind slices of 0, 1, 255, 256, 257 and 600 requests: ascending, descending, shuffled,
    one index five times; an empty slice between two with requests; two descriptors over the same bytes; requests that
    no slice names."""
    rng = np.random.default_rng(720)
    idxs = list(range(1000, 1700))
    f = source_of(rng, idxs)
    small = source_of(rng, [5, 6, 7])
    shuffled = [int(x) for x in rng.permutation(idxs)]
    reqs = [idxs[:600], [], idxs[::-1][:257], shuffled[:256], [1234] * 5, shuffled[:255], [1699], [6, 5, 7, 6]]
    files = [f, small, f, f, f, f, f, small]
    alias = {2: 0, 3: 0, 4: 0, 5: 0, 6: 0, 7: 1}
    holes = [2, 0, 0, 1, 0, 0, 3, 0, 4]
    slices, req = slices_of(reqs, holes)
    for flags in (0, VERIFY, NO_DATA):
        want = check_read(be, files, slices, req, flags, alias=alias, what=f"request shapes, flags {flags}")
        assert kinds(want) == [OK] * 8
    unnamed = [k for k in range(len(req)) if not any(a <= k < a + n for a, n in slices)]
    assert len(unnamed) == 10 and all(want["rows"][32 * k:32 * k + 32] == bytes([POISON]) * 32 for k in unnamed)


PAYLOAD_LENS = [0, 1, 15, 16, 17, 31, 33, 4097]


def check_payloads(be, width, flags):
    """Every payload length at every start alignment of the files buffer (a gap in front of each record) and at every
    start alignment of `out` (one-byte rows asked in between move it on); the lane-group width forced by padding the
    file as pad_to_width does."""
    rng = np.random.default_rng(730 + width)
    recs, pos, by = [R(1, 1, b"x")], 1, {}
    for ln in PAYLOAD_LENS:
        for phase in range(16):
            gap = (phase - pos) % 16
            by[(ln, phase)] = 100 + len(recs)
            recs.append(R(100 + len(recs), 3, rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes(), gap=gap))
            pos += gap + ln
    f = make_source(recs)
    index = ref_parse(f)
    for ln in PAYLOAD_LENS:
        assert len({index[by[(ln, ph)]][1] % 16 for ph in range(16)}) == 16
    ask, at = [], 0
    for ln in PAYLOAD_LENS:
        for a in range(16):
            while at % 16 != a:
                ask.append(1)
                at += 1
            ask.append(by[(ln, (a * 5 + 3) % 16)])
            at += ln
    files = pad_to_width([f], len(ask), width)
    slices, req = slices_of([ask])
    for src_phase, dst_phase in ((0, 0), (9, 5)):
        want = check_read(be, files, slices, req, flags, src_phase=src_phase, dst_phase=dst_phase, host_form=dst_phase == 0,
                          what=f"width {width} flags {flags} phases {src_phase}, {dst_phase}")
        assert kinds(want) == [OK]
        rows = [struct.unpack(ROW, want["rows"][32 * k:32 * k + 32]) for k in range(len(ask))]
        assert {(r[3], r[2] % 16) for r in rows if r[0] != 1} == {(ln, a) for ln in PAYLOAD_LENS for a in range(16)}


def damaged(payload):
    return bytes([payload[0] ^ 0x40]) + payload[1:]


def check_failures(be, width):
    """MISSING, TRUNCATED and Crc mismatches in every order the header ranks, with and without VERIFY, and BAD_SOURCE
    as the first, a middle and the last source: the neighbours' rows and bytes are what they are without the damage
    (the referee's answer is compared byte for byte)."""
    rng = np.random.default_rng(740 + width)
    pay = [rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes() for ln in (20, 3, 40, 17, 64, 9, 33, 16)]

    def src(spoil):
        """records 10..17; spoil {idx: 'crc' | 'zero' | 'trunc_off' | 'trunc_len'}"""
        recs = []
        for j, p in enumerate(pay):
            how = spoil.get(10 + j)
            if how == "crc":
                recs.append(R(10 + j, 1, damaged(p), crc=zlib.crc32(p)))
            elif how == "zero":
                recs.append(R(10 + j, 1, damaged(p), crc=0))
            elif how == "trunc_off":
                recs.append(R(10 + j, 1, p, off=1 << 40))
            elif how == "trunc_len":
                recs.append(R(10 + j, 1, p, ln=1 << 30))
            else:
                recs.append(R(10 + j, 1, p))
        return make_source(recs)

    good = src({})
    every = list(range(10, 18))
    cases = [
        ("missing_then_truncated", src({14: "trunc_off"}), [10, 99, 11, 14, 12], (MISSING, 1, 99), (MISSING, 1, 99)),
        ("truncated_then_missing", src({11: "trunc_len"}), [10, 11, 99, 12], (TRUNCATED, 1, 11), (TRUNCATED, 1, 11)),
        ("missing_behind_mismatch", src({10: "crc"}), [10, 11, 99], (MISSING, 2, 99), (MISSING, 2, 99)),
        ("truncated_behind_mismatch", src({10: "crc", 12: "trunc_off"}), [10, 11, 12], (TRUNCATED, 2, 12), (TRUNCATED, 2, 12)),
        ("mismatch", src({13: "crc"}), every, (OK, 8, 0), (CRC, 3, 13)),
        ("stored_crc_zero_over_damage", src({13: "zero", 15: "zero"}), every, (OK, 8, 0), (OK, 8, 0)),
        ("two_mismatches_later_record_asked_first", src({11: "crc", 16: "crc"}), [10, 16, 12, 11, 17], (OK, 5, 0), (CRC, 1, 16)),
        ("truncated_at_the_edge", src({17: "trunc_len"}), every[::-1], (TRUNCATED, 0, 17), (TRUNCATED, 0, 17)),
    ]
    files = [good] + [c[1] for c in cases] + [good]
    reqs = [every] + [c[2] for c in cases] + [every[::-1]]
    n_req = sum(len(r) for r in reqs)
    files = pad_to_width(files, n_req, width)
    slices, req = slices_of(reqs)
    for flags, col in ((0, 3), (VERIFY, 4)):
        want = check_read(be, files, slices, req, flags, what=f"failures, width {width}, flags {flags}")
        assert want["statuses"] == [(OK, 8, 0)] + [c[col] for c in cases] + [(OK, 8, 0)]
        if flags:                                       # SPACE: the same rows and results, but nothing was copied: no CRC
            short = check_read(be, files, slices, req, flags, space=True, what=f"failures, width {width}, short of room")
            assert short["statuses"] == [(OK, 8, 0)] + [c[3] for c in cases] + [(OK, 8, 0)]
            assert short["rows"] == want["rows"]
    # the exact edge of TRUNCATED: a payload that ends with the file is good, one byte more is not
    tail = make_source([R(1, 1, b"0123456789abcdef")])
    flat_len = make_source([R(1, 1, b"0123456789abcdef", ln=17)])
    at_end = make_source([R(1, 1, b"", off=len(tail), ln=0)])
    past_end = make_source([R(1, 1, b"", off=len(tail) + 1, ln=0)])
    assert len(at_end) == len(past_end) == len(tail) - 16
    at_end, past_end = at_end + bytes(16), past_end + bytes(16)
    want = check_read(be, [tail, flat_len, at_end, past_end], [(k, 1) for k in range(4)], [1] * 4, what="the edge of TRUNCATED")
    assert kinds(want) == [OK, TRUNCATED, OK, TRUNCATED]
    # BAD_SOURCE first, in the middle and last; each kind of bad header
    bads = [b"RASX" + good[4:], good[:7], good[:4] + b"\x00\x00" + good[6:], good[:4] + b"\x00\x03" + good[6:], b""]
    for place in (0, 2, 4):
        for bad in bads:
            fs = [good] * 5
            fs[place] = bad
            slices, req = slices_of([every[:3], [], every, [17, 99], every[2:5]])
            want = check_read(be, fs, slices, req, VERIFY, what=f"bad source at {place} ({len(bad)} bytes)")
            ks = kinds(want)
            assert ks[place] == BAD_SOURCE and want["statuses"][place] == (BAD_SOURCE, 0, 0)
            assert [k for s, k in enumerate(ks) if s != place] == [k for s, k in enumerate([OK, OK, OK, MISSING, OK]) if s != place]


SPREAD_REQUESTS = 600           # three steps of the resolve pass; 19 to 150 workgroups of the copy, by the lane-group width
SPREAD_POSITIONS = (330, 200, 40)   # 40 and 200: one step of the resolve pass, two wavefronts; 40 and 330: 290 apart


def check_spread_failures(be, width):
    """The SAME failure at three positions of one source's requests, far apart, the requests in DESCENDING index order
    (the later position asks for the lower-numbered record): the answer is the first position, which the kernels find
    as a minimum over atomics (s_miss_k, s_trunc_k of the resolve pass, crc_k[source] of the copy) that arrive in
    whatever order lanes and workgroups run.  Positions 40 and 200 meet in one step of the resolve pass, on different
    wavefronts; 40 and 330 lie in different workgroups of the copy.  Referee: ref_read, byte for byte."""
    n, first = SPREAD_REQUESTS, min(SPREAD_POSITIONS)
    rng = np.random.default_rng(745 + width)
    pay = [rng.integers(0, 256, size=20, dtype=np.uint8).tobytes() for _ in range(n)]
    ask = list(range(1000 + n - 1, 999, -1))                # position k asks for record 1000 + n - 1 - k
    hit = [ask[k] for k in SPREAD_POSITIONS]

    def src(how):
        recs = []
        for j, p in enumerate(pay):
            if 1000 + j not in hit or how is None:
                recs.append(R(1000 + j, 1, p))
            elif how == "crc":
                recs.append(R(1000 + j, 1, damaged(p), crc=zlib.crc32(p)))
            else:
                recs.append(R(1000 + j, 1, p, off=1 << 40))
        return make_source(recs)

    gone = list(ask)
    for k in SPREAD_POSITIONS:
        gone[k] = 99                                        # an index the file does not have
    mixed = list(ask)
    mixed[330] = 99                                         # MISSING at 330, TRUNCATED at 200 and 40 (of the "trunc" file)
    files = [src("crc"), src("trunc"), src(None), src("trunc"), src(None)]
    reqs = [ask, ask, gone, mixed, ask]
    files = pad_to_width(files, sum(len(r) for r in reqs), width)
    slices, req = slices_of(reqs)
    plain = [(OK, n, 0), (TRUNCATED, first, ask[first]), (MISSING, first, 99), (TRUNCATED, first, ask[first]), (OK, n, 0)]
    for flags in (0, VERIFY):
        want = check_read(be, files, slices, req, flags, host_form=False, what=f"spread failures, width {width}, flags {flags}")
        assert want["statuses"] == ([(CRC, first, ask[first])] if flags else plain[:1]) + plain[1:]


def check_sizing_and_modes(be):
    rng = np.random.default_rng(750)
    f0, f1 = source_of(rng, list(range(1, 40))), source_of(rng, list(range(50, 90)))
    slices, req = slices_of([[3, 4, 5, 99, 30], list(range(89, 49, -1))])
    sources, buf = pack_read([f0, f1], slices)
    # the sizing call: out = NULL, out_bytes = 0 ...
    want0 = ref_read([f0, f1], sources, req, 0, 0)
    rows, results, total, _ = device_read(be, sources, buf, req, 0, 0, null_out=True)
    assert want0["space"] and (rows, results, total) == (want0["rows"], want0["results"], want0["total"])
    needed = struct.unpack("<IIQ", total)[2]
    assert needed == want0["needed"] > 0
    # ... needed - 1 is still SPACE, with the whole of out untouched; needed itself is enough
    check_read(be, [f0, f1], slices, req, space=True, what="needed - 1")
    check_read(be, [f0, f1], slices, req, slack=0, what="exactly needed")
    check_read(be, [f0, f1], slices, req, VERIFY, slack=0, dst_phase=3, what="exactly needed, verify")
    # the host form sizes by itself
    tot, res, h_rows, data = be.eng.segment_read(sources, buf, req)
    full = ref_read([f0, f1], sources, req)
    assert (tot.tobytes(), res.tobytes(), h_rows.tobytes(), data.tobytes()) == (full["total"], full["results"], full["rows"], full["out"])
    # NO_DATA with out = NULL: rows only, offsets into the files buffer, never SPACE
    want = ref_read([f0, f1], sources, req, NO_DATA, 0)
    rows, results, total, _ = device_read(be, sources, buf, req, NO_DATA, 0, null_out=True)
    assert (rows, results, total) == (want["rows"], want["results"], want["total"])
    assert struct.unpack("<IIQ", total) == (OK, 1, 0)
    for k in (0, 1, 2, 4):
        idx, term, off, ln, crc = struct.unpack(ROW, rows[32 * k:32 * k + 32])
        assert zlib.crc32(buf[off:off + ln].tobytes()) == crc and off != UNDEF
    tot, res, h_rows, data = be.eng.segment_read(sources, buf, req, NO_DATA)
    assert (tot.tobytes(), h_rows.tobytes(), len(data)) == (want["total"], want["rows"], 0)
    # no sources; sources without requests (the header is still looked at)
    check_read(be, [], [], [], what="no sources")
    check_read(be, [], [], [1, 2, 3], what="no sources, requests of nobody")
    want = check_read(be, [f0, b"RASG", f1], [(0, 0)] * 3, [], what="no requests")
    assert kinds(want) == [OK, BAD_SOURCE, OK]
    # payloads of length 0 only: nothing is needed, out may be NULL without NO_DATA
    z = make_source([R(1, 1), R(2, 1)])
    sources, buf = pack_read([z], [(0, 2)])
    want = ref_read([z], sources, [2, 1], VERIFY, 0)
    assert (want["space"], want["needed"]) == (False, 0)
    rows, results, total, _ = device_read(be, sources, buf, np.array([2, 1], dtype=np.uint64), VERIFY, 0, null_out=True)
    assert (rows, results, total) == (want["rows"], want["results"], want["total"])


def check_many_sources(be):
    """300 one-record sources: the place pass crosses its own step; source 256 is bad, 257 has a mismatch."""
    rng = np.random.default_rng(760)
    files, reqs = [], []
    for s in range(300):
        p = rng.integers(0, 256, size=int(rng.integers(0, 40)), dtype=np.uint8).tobytes()
        files.append(make_source([R(1000 + s, s + 1, p if s != 257 else damaged(p + b"!"),
                                    crc=None if s != 257 else zlib.crc32(p + b"!"))]))
        reqs.append([1000 + s] if s % 50 else [1000 + s, 7])
    files[256] = b"RASG\x00\x09" + files[256][6:]
    slices, req = slices_of(reqs)
    for flags in (0, VERIFY):
        want = check_read(be, files, slices, req, flags, host_form=bool(flags), what=f"300 sources, flags {flags}")
        ks = kinds(want)
        assert ks[256] == BAD_SOURCE and ks[257] == (CRC if flags else OK) and ks[255] == ks[258] == OK
        assert ks.count(MISSING) == 6 and struct.unpack("<IIQ", want["total"])[1] == (8 if flags else 7)


def check_composition(be):
    """The rows and `out` of a read, handed unchanged to rgb_segment_build, give the image python_segment gives for the
    same entries."""
    rng = np.random.default_rng(770)
    idxs = list(range(20, 60))
    pay = [rng.integers(0, 256, size=int(ln), dtype=np.uint8).tobytes() for ln in rng.integers(0, 300, size=len(idxs))]
    f = make_source([R(i, 7 + i % 3, p) for i, p in zip(idxs, pay)], version=1)
    ask = [59, 20, 33, 33, 41] + idxs[5:25]
    sources, buf = pack_read([f], [(0, len(ask))])
    tot, res, rows, data = be.eng.segment_read(sources, buf, ask, VERIFY)
    assert int(tot["status"]) == OK and int(res["status"][0]) == OK
    image = be.eng.segment_build(rows, data, len(ask) + 2)
    want = python_segment([(i, 7 + i % 3) for i in ask], [pay[i - 20] for i in ask], len(ask) + 2)
    assert first_diff(image.tobytes(), want) is None


FUZZ_CASES = 120               # kept cases per call of check_fuzz (nothing is discarded: every drawn case is run)


def random_case(rng):
    n_src = int(rng.integers(1, 6))
    files, reqs, holes = [], [], []
    for s in range(n_src):
        n = int(rng.choice([0, 1, 3, 8, 20, 40]))
        seq, cur = [], int(rng.integers(1, 50))
        for _ in range(n):
            cur = max(1, cur + int(rng.choice([1, 1, 1, 1, 2, 0, -3, -7])))
            seq.append(cur)
        recs = []
        for j, i in enumerate(seq):
            p = rng.integers(0, 256, size=int(rng.choice([0, 1, 5, 15, 16, 17, 40, 100])), dtype=np.uint8).tobytes()
            how = int(rng.integers(0, 20))
            if how == 0 and p:
                recs.append(R(i, j + 1, damaged(p), crc=zlib.crc32(p)))
            elif how == 1 and p:
                recs.append(R(i, j + 1, damaged(p), crc=0))
            elif how == 2:
                recs.append(R(i, j + 1, p, off=10 ** 6))
            elif how == 3:
                recs.append(R(i, j + 1, p, ln=len(p) + int(rng.choice([1, 60, 5000]))))
            else:
                recs.append(R(i, j + 1, p))
        f = make_source(recs, max_count=n + int(rng.integers(0, 3)), version=2 if rng.integers(0, 4) else 1,
                        tail=int(rng.integers(0, 4)))
        if rng.integers(0, 12) == 0:
            f = (b"RASX" + f[4:], f[:5], f[:4] + b"\x00\x07" + f[6:])[int(rng.integers(0, 3))]
        files.append(f)
        pool = seq + [0, 1000, max(seq + [1]) + 1]
        reqs.append([int(rng.choice(pool)) for _ in range(int(rng.choice([0, 1, 2, 5, 12, 30])))])
        holes.append(int(rng.integers(0, 3)) if rng.integers(0, 3) == 0 else 0)
    holes.append(int(rng.integers(0, 2)))
    return files, reqs, holes, int(rng.choice([0, VERIFY, NO_DATA])), bool(rng.integers(0, 6) == 0)


def check_fuzz(be, seed, count=FUZZ_CASES):
    """Random sources and requests against the referee, fixed seeds.  The generator discards nothing: `count` cases
    are drawn and `count` are kept and run (a drawn SPACE case whose read needs no bytes runs with room instead)."""
    rng = np.random.default_rng(seed)
    drawn = kept = 0
    seen = set()
    for trial in range(count):
        files, reqs, holes, flags, space = random_case(rng)
        drawn += 1
        slices, req = slices_of(reqs, holes)
        sources, _ = pack_read(files, slices)
        if space and (flags & NO_DATA or ref_read(files, sources, req, flags)["needed"] == 0):
            space = False
        want = check_read(be, files, slices, req, flags, space, src_phase=trial % 16, dst_phase=(trial * 7) % 16,
                          host_form=trial % 4 == 0, what=f"seed {seed} trial {trial}")
        kept += 1
        seen.update(kinds(want))
        seen.add("space" if want["space"] else "room")
    assert kept * 10 >= drawn * 9 and kept == count
    assert seen >= {OK, MISSING, TRUNCATED, CRC, BAD_SOURCE, "space", "room"}, seen


def check_refusals(be):
    """Every RGB_E_INVAL of the header leaves rows, out, results and total untouched, in both forms."""
    rng = np.random.default_rng(780)
    f = source_of(rng, [1, 2, 3])
    req = np.array([1, 2, 3, 1, 2, 3], dtype=np.uint64)
    good, buf = pack_read([f, f], [(0, 3), (3, 3)])

    def rows_of(**kw):
        s = good.copy()
        for k, (i, v) in kw.items():
            s[k][i] = v
        return s

    many = np.zeros(abi.SEG_READ_MAX_SOURCES + 1, dtype=abi.SEG_READ_SOURCE_DTYPE)
    cases = [("slice outside n_req", rows_of(req_n=(1, 4)), 0, len(buf)),
             ("slice starts outside n_req", rows_of(req_first=(1, 7), req_n=(1, 0)), 0, len(buf)),
             ("slices not ascending", good[::-1].copy(), 0, len(buf)),
             ("slices overlap", rows_of(req_first=(1, 2)), 0, len(buf)),
             ("source outside files_bytes", good, 0, len(buf) - 6),
             ("source offset outside", rows_of(offset=(0, 1 << 62)), 0, len(buf)),
             ("n_bytes wraps", rows_of(n_bytes=(0, UNDEF)), 0, len(buf)),
             ("unknown flag", good, 4, len(buf)),
             ("verify with no_data", good, VERIFY | NO_DATA, len(buf)),
             ("too many sources", many, 0, len(buf))]
    for name, sources, flags, files_bytes in cases:
        d_f, p_f, _ = be.dev(buf)
        d_w, p_w, b_w = be.dev(guarded(32 * len(req)))
        d_o, p_o, b_o = be.dev(guarded(500))
        d_r, p_r, b_r = be.dev(np.full(32 * 2, 0x77, dtype=np.uint8))
        d_t, p_t, b_t = be.dev(np.full(16, 0x77, dtype=np.uint8))
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.segment_read_device(sources, p_f, files_bytes, req, p_w + GUARD, p_o + GUARD, 500, p_r, p_t, flags)
        assert e.value.code == E_INVAL, name
        be.sync()
        assert inside(be.get(d_w), b_w, 32 * len(req), "d_rows") == bytes([POISON]) * (32 * len(req)), name
        assert inside(be.get(d_o), b_o, 500, "d_out") == bytes([POISON]) * 500, name
        assert np.all(be.get(d_r)[b_r:b_r + 64] == 0x77) and np.all(be.get(d_t)[b_t:b_t + 16] == 0x77), name
        h_rows = np.full(32 * len(req), POISON, dtype=np.uint8).view(abi.SEG_ENTRY_DTYPE)
        h_out = np.full(500, POISON, dtype=np.uint8)
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.segment_read(sources, buf[:files_bytes], req, flags, rows=h_rows, out=h_out)
        assert e.value.code == E_INVAL, name
        assert np.all(h_rows.view(np.uint8) == POISON) and np.all(h_out == POISON), name
    # the good descriptors of the same call are served
    want = check_read(be, [f, f], [(0, 3), (3, 3)], req, what="the good call")
    assert kinds(want) == [OK, OK]


def check_back_to_back_calls(be):
    """Calls enqueued behind each other on one context (the pinned descriptors and the scratch are reused): a large
    read, then a small one, then the large one again, answers fetched afterwards."""
    rng = np.random.default_rng(790)
    big = [source_of(rng, list(range(1, 300))) for _ in range(3)]
    small = [source_of(rng, [4, 5])]
    calls = [(big, [list(range(299, 0, -1))] * 3, VERIFY), (small, [[5, 4, 9]], 0), (big, [[7] * 300, [], [1, 2]], 0)]
    pending = []
    for files, reqs, flags in calls:
        slices, req = slices_of(reqs)
        sources, buf = pack_read(files, slices)
        want = ref_read(files, sources, req, flags)
        out_bytes = want["needed"] + 8
        d_f, p_f, _ = be.dev(buf)
        d_w, p_w, b_w = be.dev(guarded(32 * len(req)))
        d_o, p_o, b_o = be.dev(guarded(out_bytes))
        d_r, p_r, b_r = be.dev(np.full(32 * len(files), 0x77, dtype=np.uint8))
        d_t, p_t, b_t = be.dev(np.full(16, 0x77, dtype=np.uint8))
        be.eng.segment_read_device(sources, p_f, len(buf), req, p_w + GUARD, p_o + GUARD, out_bytes, p_r, p_t, flags)
        pending.append((want, out_bytes, len(req), len(files), d_f, (d_w, b_w), (d_o, b_o), (d_r, b_r), (d_t, b_t)))
    for c, (want, out_bytes, n_req, n_src, _, (d_w, b_w), (d_o, b_o), (d_r, b_r), (d_t, b_t)) in enumerate(pending):
        same(inside(be.get(d_w), b_w, 32 * n_req, "d_rows"), want["rows"], f"call {c}: rows")
        same(inside(be.get(d_o), b_o, out_bytes, "d_out"), want["out"] + bytes([POISON]) * 8, f"call {c}: out")
        same(be.get(d_r)[b_r:b_r + 32 * n_src].tobytes(), want["results"], f"call {c}: results")
        same(be.get(d_t)[b_t:b_t + 16].tobytes(), want["total"], f"call {c}: total")


# ------------------------------------------------------------------------------------------ CPU (emulation)

def test_abi_mirror():
    hdr = " ".join(open(os.path.join(ROOT, "include", "ra_gpu_wal.h")).read().split())
    for name, val in (("RGB_SEG_READ_OK", abi.SEG_READ_OK), ("RGB_SEG_READ_MISSING", abi.SEG_READ_MISSING),
                      ("RGB_SEG_READ_TRUNCATED", abi.SEG_READ_TRUNCATED), ("RGB_SEG_READ_CRC", abi.SEG_READ_CRC),
                      ("RGB_SEG_READ_BAD_SOURCE", abi.SEG_READ_BAD_SOURCE), ("RGB_SEG_READ_SPACE", abi.SEG_READ_SPACE),
                      ("RGB_SEG_READ_VERIFY", abi.SEG_READ_VERIFY), ("RGB_SEG_READ_NO_DATA", abi.SEG_READ_NO_DATA),
                      ("RGB_SEG_READ_MAX_SOURCES", abi.SEG_READ_MAX_SOURCES)):
        assert int(hdr.split(f"#define {name} ")[1].split()[0].rstrip("u")) == val, name
    assert (OK, MISSING, TRUNCATED, CRC, BAD_SOURCE, SPACE) == (abi.SEG_READ_OK, abi.SEG_READ_MISSING, abi.SEG_READ_TRUNCATED,
                                                                abi.SEG_READ_CRC, abi.SEG_READ_BAD_SOURCE, abi.SEG_READ_SPACE)
    assert "#define RGB_ABI_VERSION 10u" in " ".join(open(os.path.join(ROOT, "include", "ra_gpu_batch.h")).read().split())
    assert (abi.SEG_READ_SOURCE_DTYPE.itemsize, abi.SEG_READ_RESULT_DTYPE.itemsize, abi.SEG_READ_TOTAL_DTYPE.itemsize) == (32, 32, 16)
    assert abi.SEG_READ_SOURCE_DTYPE.itemsize == abi.SEG_SOURCE_DTYPE.itemsize
    assert [abi.SEG_READ_SOURCE_DTYPE.fields[k][1] for k in ("offset", "n_bytes", "req_first", "req_n")] == [0, 8, 16, 20]
    assert [abi.SEG_READ_RESULT_DTYPE.fields[k][1] for k in ("status", "n_read", "index", "data_bytes")] == [0, 4, 8, 16]
    assert [abi.SEG_READ_TOTAL_DTYPE.fields[k][1] for k in ("status", "n_bad", "out_bytes")] == [0, 4, 8]
    assert struct.calcsize(ROW) == abi.SEG_ENTRY_DTYPE.itemsize == 32
    assert STEP == int(open(os.path.join(ROOT, "ra_amd", "csrc", "rgb_segment.hip")).read().split("constexpr int THREADS = ")[1].split(";")[0])


@pytest.mark.parametrize("n", SOURCE_SIZES)
def test_emu_source_sizes(emu, n):
    check_source_sizes(emu, n)


def test_emu_index_shapes(emu):
    check_index_shapes(emu)


def test_emu_request_shapes(emu):
    check_request_shapes(emu)


@pytest.mark.parametrize("flags", [0, VERIFY], ids=["plain", "verify"])
@pytest.mark.parametrize("width", [8, 16, 64])
def test_emu_payloads(emu, width, flags):
    check_payloads(emu, width, flags)


@pytest.mark.parametrize("width", [8, 16, 64])
def test_emu_failures(emu, width):
    check_failures(emu, width)


@pytest.mark.parametrize("width", [8, 16, 64])
def test_emu_spread_failures(emu, width):
    check_spread_failures(emu, width)


@pytest.mark.parametrize("sched", PERMUTED_SCHEDULES)
def test_emu_under_permuted_schedules(emu, sched):
    """The emulation's own order is workgroups 0, 1, 2, ... and lanes 0 .. 255, so "the first failing position", which
    the kernels take as a minimum over atomics, also arrives first.  The checks that reach those atomics once more with
    workgroups and lanes reversed and permuted (tests/emu_schedule.py); the referee stays ref_read."""
    with schedule(emu.engine, sched):
        for width in (8, 16, 64):
            check_failures(emu, width)
            check_spread_failures(emu, width)
        check_many_sources(emu)
        check_composition(emu)
        check_fuzz(emu, 7900)


def test_emu_sizing_and_modes(emu):
    check_sizing_and_modes(emu)


def test_emu_many_sources(emu):
    check_many_sources(emu)


def test_emu_composition(emu):
    check_composition(emu)


@pytest.mark.parametrize("seed", [7900, 7901])
def test_emu_fuzz(emu, seed):
    check_fuzz(emu, seed)


def test_emu_refusals(emu):
    check_refusals(emu)


def test_emu_back_to_back_calls(emu):
    check_back_to_back_calls(emu)


def test_read_descriptors_under_sanitizers(tmp_path):
    """rgb_seg_read_check -- the host-side validation of every read call, in the host-only unit rgb_segment_host.cpp --
    compiled with AddressSanitizer + UBSan into a stand-alone program and run over malformed and good descriptors, each
    array in an exactly-sized heap block."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"                      # is the sanitizer runtime there at all?
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=address,undefined", "-o", str(tmp_path / "probe"), str(probe)],
                      capture_output=True).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    exe = tmp_path / "segment_read_harness"
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-o", str(exe),
           os.path.join(ROOT, "tests", "native", "segment_read_harness.cpp"),
           os.path.join(ROOT, "ra_amd", "csrc", "rgb_segment_host.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def rows(*r):
        s = np.zeros(len(r), dtype=abi.SEG_READ_SOURCE_DTYPE)
        for k, (off, nb, first, n) in enumerate(r):
            s["offset"][k], s["n_bytes"][k], s["req_first"][k], s["req_n"][k] = off, nb, first, n
        return s

    big = 1 << 63
    cases = [  # sources, n_req, files_bytes, flags -> rc, covered, sum of n_bytes, bound
        (rows((0, 100, 0, 3), (100, 50, 3, 0), (20, 30, 5, 2)), 9, 150, 0, 0, 5, 180, 360),
        (rows(), 0, 0, 0, 0, 0, 0, 0),
        (rows(), 0xFFFFFFFF, UNDEF, VERIFY, 0, 0, 0, 0),
        (rows((0, 0, 0xFFFFFFFF, 0)), 0xFFFFFFFF, 0, NO_DATA, 0, 0, 0, 0),
        (rows((0, big, 0, 0xFFFFFFFF), (big - 1, big, 0xFFFFFFFF, 0)), 0xFFFFFFFF, UNDEF, 0, 0, 0xFFFFFFFF, UNDEF, UNDEF),
        (rows((0, 100, 0, 4)), 3, 100, 0, E_INVAL, 0, 0, 0),
        (rows((0, 100, 4, 0)), 3, 100, 0, E_INVAL, 0, 0, 0),
        (rows((0, 100, 2, 2), (0, 100, 0, 2)), 4, 100, 0, E_INVAL, 0, 0, 0),
        (rows((0, 100, 0, 3), (0, 100, 2, 1)), 4, 100, 0, E_INVAL, 0, 0, 0),
        (rows((1, 100, 0, 1)), 1, 100, 0, E_INVAL, 0, 0, 0),
        (rows((UNDEF, 1, 0, 1)), 1, 100, 0, E_INVAL, 0, 0, 0),
        (rows((1, UNDEF, 0, 1)), 1, UNDEF, 0, E_INVAL, 0, 0, 0),
        (rows((0, 100, 0, 1)), 1, 100, 4, E_INVAL, 0, 0, 0),
        (rows((0, 100, 0, 1)), 1, 100, VERIFY | NO_DATA, E_INVAL, 0, 0, 0),
        (np.zeros(abi.SEG_READ_MAX_SOURCES, dtype=abi.SEG_READ_SOURCE_DTYPE), 0, 0, 0, 0, 0, 0, 0),
        (np.zeros(abi.SEG_READ_MAX_SOURCES + 1, dtype=abi.SEG_READ_SOURCE_DTYPE), 0, 0, 0, E_INVAL, 0, 0, 0),
    ]
    files = []
    for k, (s, n_req, fb, flags, *_) in enumerate(cases):
        path = tmp_path / f"r{k}.bin"
        path.write_bytes(struct.pack("<IIQII", len(s), n_req, fb, flags, 0) + s.tobytes())
        files.append(str(path))
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in run.stdout.splitlines()]
    assert got == [c[4:] for c in cases]


def test_read_kernels_resources():
    """hipcc's resource remarks for gfx950 (no GPU needed), as tests/test_kernel_resources.py reads them.  The kernels
    whose names contain rgb_read_ are the nine of this feature: resolve, place, finish and the copy for 3 widths x
    {verify, plain}.  None uses scratch or spills; LDS within the 20 KiB (+ 64) the unit's other gates allow, the plain
    copy without the CRC tables; every one reaches at least the occupancy of rgb_compact_resolve_kernel, which the
    factoring of the index walk left as it was at the commit before (44 VGPRs, 11288 bytes of LDS, 8 wavefronts)."""
    from test_kernel_resources import segment_usage
    usage = segment_usage()
    (resolve,) = [k for k in usage if "rgb_compact_resolve_kernel" in k]
    floor = usage[resolve]["Occupancy"]
    assert (usage[resolve]["VGPRs"], usage[resolve]["LDS Size"], floor) == (44, 11288, 8), usage[resolve]
    names = sorted(k for k in usage if "rgb_read_" in k)
    want = ["rgb_read_resolve_kernel", "rgb_read_place_kernel", "rgb_read_finish_kernel"] + \
           [f"rgb_read_copy_kernelILi{g}ELb{v}E" for g in (8, 16, 64) for v in (0, 1)]
    assert len(names) == 9 and all(sum(w in k for k in names) == 1 for w in want), names
    for k in names:
        u = usage[k]
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, f"{k}: {u}"
        assert u["LDS Size"] <= 20 * 1024 + 64, f"{k}: {u}"
        assert u["Occupancy"] >= floor, f"{k}: {u}"
        if "copy_kernel" in k and "ELb0E" in k:             # <GROUP, VERIFY = false>
            assert u["LDS Size"] <= 64, f"{k}: the plain copy must not hold the CRC tables"
    assert all("rgb_seg_" not in k and "rgb_compact_" not in k and "rgb_flush_" not in k for k in names)


# ------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("n", SOURCE_SIZES)
def test_gpu_source_sizes(gpu, n):
    check_source_sizes(gpu, n)


@pytest.mark.gpu
def test_gpu_index_shapes(gpu):
    check_index_shapes(gpu)


@pytest.mark.gpu
def test_gpu_request_shapes(gpu):
    check_request_shapes(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, VERIFY], ids=["plain", "verify"])
@pytest.mark.parametrize("width", [8, 16, 64])
def test_gpu_payloads(gpu, width, flags):
    check_payloads(gpu, width, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [8, 16, 64])
def test_gpu_failures(gpu, width):
    check_failures(gpu, width)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [8, 16, 64])
def test_gpu_spread_failures(gpu, width):
    check_spread_failures(gpu, width)


@pytest.mark.gpu
def test_gpu_sizing_and_modes(gpu):
    check_sizing_and_modes(gpu)


@pytest.mark.gpu
def test_gpu_many_sources(gpu):
    check_many_sources(gpu)


@pytest.mark.gpu
def test_gpu_composition(gpu):
    check_composition(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [7900, 7901])
def test_gpu_fuzz(gpu, seed):
    check_fuzz(gpu, seed)


@pytest.mark.gpu
def test_gpu_refusals(gpu):
    check_refusals(gpu)


@pytest.mark.gpu
def test_gpu_back_to_back_calls(gpu):
    check_back_to_back_calls(gpu)
