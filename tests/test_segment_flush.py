"""Batched mem-table flush: rgb_segment_flush_bound / rgb_segment_flush_device / rgb_segment_flush (include/ra_gpu_wal.h,
"mem-table flush"; ra_amd/csrc/rgb_segment.hip, rgb_segment_host.cpp).

Referee: a sequential pure-Python restatement, written from the reference source, of
  ref_append   ra_log_segment:append/4          src/ra_log_segment.erl:252-292 (is_full/1 :1250-1255 tested first,
                                                DataOffset and the index record, update_range/2 :919-922)
               + flush/1                        :316-338 (the pending index and data bytes written where they belong)
  ref_flush    append_to_segment/6              src/ra_log_segment_writer.erl:425-500: on {error, full} a successor is
                                                opened with the configured MaxCount and the entry appended to it
with struct.pack and zlib.crc32.  It keeps a list of file images per writer and appends entry by entry; the library
splits by prefix sums and a walk over segments -- the referee deliberately does not.  The library's answer is checked
by APPLYING it: from the same open-segment images (tests/test_segment.py::python_segment, the count set by hand) the
two writes of every piece are performed and every file compared byte for byte with the referee's; then the piece rows
and the result row are compared.

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
from test_segment import Emu, Gpu, emu, gpu, first_diff, force_group, python_segment          # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL = -1
OK, SPACE, ENTRY = range(3)
NO_CRC = abi.SEG_NO_CHECKSUMS
UNDEF = (1 << 64) - 1
CHUNK = 64                     # rgb_segment.hip: entries of a writer per step of the plan pass (FL_CHUNK)
GUARD = 64
BIG = 1 << 40                  # a max_size nothing here reaches
# hipcc's resource remarks for rgb_seg_crc_kernel<GROUP, true> at the commit before this feature (the kernels the copy
# pass is measured against): GROUP -> (Occupancy, LDS Size)
PARENT_BUILD_KERNELS = {8: (8, 20480), 16: (8, 20480), 64: (7, 20480)}


# ------------------------------------------------------------------------------------------ referee

class RefFile:
    """One segment file: its bytes and what the reference's #state{} knows of it.  `hole`: payload bytes the open file
    is said to hold that the image does not (an open_data_bytes beyond 2^32 needs no data there): file offsets behind
    the image's own end are moved down by it."""

    def __init__(self, max_count, image=None, count=0, data_bytes=0, rng=None, hole=0):
        self.max_count, self.data_start = max_count, 8 + 32 * max_count
        self.image = bytearray(struct.pack(">4sHH", b"RASG", 2, max_count) if image is None else image)
        self.count, self.data_offset, self.range = count, self.data_start + data_bytes + hole, rng
        self.hole, self.hole_at = hole, len(self.image)
        self.appended, self.appended_bytes = [], 0          # by this flush: entry numbers, payload bytes

    def copy(self):
        f = RefFile(self.max_count, bytes(self.image), self.count, 0, self.range, self.hole)
        f.data_offset = self.data_offset
        return f

    def pwrite(self, off, data):
        if not data:
            return
        if self.hole and off >= self.data_start:
            assert off >= self.hole_at + self.hole, "a write into bytes the file is said to hold already"
            off -= self.hole
        if len(self.image) < off + len(data):
            self.image += bytes(off + len(data) - len(self.image))
        self.image[off:off + len(data)] = data


def ref_append(f, e_no, idx, term, payload, max_size, checksums):
    if f.count >= f.max_count or f.data_offset - f.data_start > max_size:        # is_full/1: "greater than"
        return False                                                             # {error, full}
    crc = zlib.crc32(payload) if checksums else 0
    f.pwrite(8 + 32 * f.count, struct.pack(">QQQII", idx, term, f.data_offset, len(payload), crc))
    f.pwrite(f.data_offset, payload)
    f.count, f.data_offset = f.count + 1, f.data_offset + len(payload)
    f.range = (idx, idx) if f.range is None else (min(f.range[0], idx), idx)     # update_range/2: the last index wins
    f.appended.append(e_no)
    f.appended_bytes += len(payload)
    return True


def ref_flush(opens, batches, max_count, max_size, checksums=True):
    """opens[w]: the open file (changed in place); batches[w]: [(entry number, Idx, Term, payload)] -> files per writer"""
    out = []
    for f, batch in zip(opens, batches):
        files = [f]
        for e_no, idx, term, payload in batch:
            if not ref_append(files[-1], e_no, idx, term, payload, max_size, checksums):
                files.append(RefFile(max_count))
                assert ref_append(files[-1], e_no, idx, term, payload, max_size, checksums)
        out.append(files)
    return out


def ref_pieces(files_per_writer):
    """The piece rows the referee's files imply, with their places in the packed `out`; -> (rows, out_bytes)"""
    rows, pos = [], 0
    for w, files in enumerate(files_per_writer):
        for k, f in enumerate(files):
            if not f.appended:
                continue
            n = len(f.appended)
            if k:
                pos += 8
            row = dict(writer=w, ordinal=k, entry_first=f.appended[0], entry_n=n, index_file_off=8 + 32 * (f.count - n),
                       data_file_off=f.data_offset - f.appended_bytes, out_index_off=pos, out_data_off=pos + 32 * n,
                       data_bytes=f.appended_bytes, range_first=f.range[0], range_last=f.range[1], max_count=f.max_count)
            assert f.appended == list(range(f.appended[0], f.appended[0] + n))
            pos += 32 * n + f.appended_bytes
            rows.append(row)
    return rows, pos


def apply_pieces(opens, pieces, out):
    """Exactly the two writes per piece (a successor's first write starts with its header, at offset 0)."""
    files = [[f] for f in opens]
    for p in pieces:
        w, k, n = int(p["writer"]), int(p["ordinal"]), int(p["entry_n"])
        io, do, db = int(p["out_index_off"]), int(p["out_data_off"]), int(p["data_bytes"])
        lst = files[w]
        assert k >= len(lst) - 1 and n >= 1, "pieces of a writer out of order, or an empty piece"
        if k == 0:
            assert not lst[0].appended
            lst[0].appended = [0]                         # (a second piece for the open file is refused above)
            lst[0].pwrite(int(p["index_file_off"]), out[io:io + 32 * n])
        else:
            assert k == len(lst), f"writer {w}: ordinal {k} after {len(lst) - 1}"
            assert int(p["index_file_off"]) == 8
            lst.append(RefFile(int(p["max_count"]), b""))
            lst[k].pwrite(0, out[io - 8:io + 32 * n])
        lst[k].pwrite(int(p["data_file_off"]), out[do:do + db])
    return files


# ------------------------------------------------------------------------------------------ building inputs

def rnd_bytes(rng, n):
    return rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes()


def mk_writer(rng, lens, omax=8, ocount=0, olens=None, hole=0, oidx=100, idxs=None, terms=None):
    """One writer: an open segment of `ocount` records (payload lengths `olens`, indexes from `oidx`) with MaxCount
    `omax`, and the entries to flush (ascending behind the open range unless `idxs` says otherwise)."""
    olens = [5] * ocount if olens is None else olens
    assert len(olens) == ocount <= omax
    opay = [rnd_bytes(rng, ln) for ln in olens]
    image = python_segment([(oidx + j, 1) for j in range(ocount)], opay, omax)
    rng_open = (oidx, oidx + ocount - 1) if ocount else None
    idxs = [oidx + ocount + j for j in range(len(lens))] if idxs is None else idxs
    terms = [2] * len(lens) if terms is None else terms
    return dict(open=RefFile(omax, image, ocount, sum(olens), rng_open, hole),
                entries=[(i, t, rnd_bytes(rng, ln)) for i, t, ln in zip(idxs, terms, lens)])


def build_call(rng, specs, phases=None, gaps=False, tail=0):
    """-> (writers, entries, data, batches): the entries of all writers in one array (with `gaps`, entries that no
    writer names in between), the payloads in one data buffer, each at a chosen address phase mod 16 (`phases`, per
    entry) or behind a random gap."""
    writers = np.zeros(len(specs), dtype=abi.SEG_WRITER_DTYPE)
    rows, batches = [], []
    for w, s in enumerate(specs):
        if gaps:
            rows += [(7, 7, rnd_bytes(rng, rng.integers(0, 30)))] * int(rng.integers(0, 3))
        f = s["open"]
        writers[w] = (len(rows), len(s["entries"]), f.count, f.max_count, f.data_offset - f.data_start,
                      f.range[0] if f.range else UNDEF, f.range[1] if f.range else UNDEF, 0)
        batches.append([(len(rows) + j, i, t, p) for j, (i, t, p) in enumerate(s["entries"])])
        rows += s["entries"]
    if gaps:
        rows += [(9, 9, b"xyz")]
    entries = np.zeros(len(rows), dtype=abi.SEG_ENTRY_DTYPE)
    chunks, pos = [], 0
    for j, (idx, term, p) in enumerate(rows):
        pad = int(rng.integers(0, 7)) if phases is None else (phases[j] - pos) % 16
        chunks.append(bytes(pad)); pos += pad
        entries[j] = (idx, term, pos, len(p), 0xDEADBEEF)             # crc: ignored on input
        chunks.append(p); pos += len(p)
    data = np.frombuffer(b"".join(chunks) + bytes(tail), dtype=np.uint8).copy()
    return writers, entries, data, batches


# ------------------------------------------------------------------------------------------ calling the library

def device_flush(be, writers, entries, data, max_count, max_size, flags=0, pieces_cap=None, out_bytes=None,
                 src_phase=0, dst_phase=0):
    """-> (result record, the pieces_cap rows of d_pieces as bytes, the out_bytes of d_out); both buffers are poisoned
    first and the guard bytes in front of and behind them are checked."""
    call, fetch = prepared_flush(be, writers, entries, data, max_count, max_size, flags, pieces_cap, out_bytes,
                                 src_phase, dst_phase)
    call()
    return fetch()


def prepared_flush(be, writers, entries, data, max_count, max_size, flags=0, pieces_cap=None, out_bytes=None,
                   src_phase=0, dst_phase=0):
    """-> (call, fetch): the buffers of one rgb_segment_flush_device call are on the device; call() enqueues it,
    fetch() waits and returns what device_flush returns."""
    out_bound, pieces_bound = be.engine.segment_flush_bound(writers, len(entries), len(data))
    assert (out_bound, pieces_bound) == (len(data) + 40 * len(entries), len(entries))
    pieces_cap = pieces_bound + 2 if pieces_cap is None else pieces_cap
    out_bytes = out_bound + 48 if out_bytes is None else out_bytes
    guard = np.full(GUARD, 0xC3, dtype=np.uint8)
    arr_o = np.concatenate([guard, np.full(out_bytes, 0xEE, dtype=np.uint8), guard])
    arr_p = np.concatenate([guard, np.full(80 * pieces_cap, 0xEE, dtype=np.uint8), guard])
    d_e, p_e, _ = be.dev(entries.view(np.uint8))
    d_d, p_d, _ = be.dev(data, src_phase)
    d_o, p_o, b_o = be.dev(arr_o, dst_phase)
    d_p, p_p, b_p = be.dev(arr_p)
    d_r, p_r, b_r = be.dev(np.full(32, 0x77, dtype=np.uint8))

    def call():
        be.eng.segment_flush_device(writers, p_e, len(entries), p_d, len(data), p_p + GUARD, pieces_cap, p_o + GUARD,
                                    out_bytes, p_r, max_count, max_size, flags)

    def fetch(_keep=(d_e, d_d)):                            # (the inputs live until the answer has been read)
        got_o, got_p = be.get(d_o), be.get(d_p)
        res = be.get(d_r)[b_r:b_r + 32].copy().view(abi.SEG_FLUSH_RESULT_DTYPE)[0]
        for got, base, arr, name in ((got_o, b_o, arr_o, "d_out"), (got_p, b_p, arr_p, "d_pieces")):
            assert np.all(got[:base] == 0) and np.all(got[base + len(arr):] == 0), f"wrote outside the buffer of {name}"
            assert np.all(got[base:base + GUARD] == 0xC3), f"wrote in front of {name}"
            assert np.all(got[base + len(arr) - GUARD:base + len(arr)] == 0xC3), f"wrote behind {name}"
        return res, got_p[b_p + GUARD:b_p + GUARD + 80 * pieces_cap].copy(), \
            got_o[b_o + GUARD:b_o + GUARD + out_bytes].copy()
    return call, fetch


ROW_FIELDS = ("writer", "ordinal", "entry_first", "entry_n", "index_file_off", "data_file_off", "out_index_off",
              "out_data_off", "data_bytes", "range_first", "range_last", "max_count")


def check_answer(specs, batches, max_count, max_size, flags, res, pieces, out, what):
    """The answer applied to copies of the open images against the referee's files, then the rows and the result."""
    want_files = ref_flush([s["open"].copy() for s in specs], batches, max_count, max_size, not flags & NO_CRC)
    want_rows, want_bytes = ref_pieces(want_files)
    assert int(res["status"]) == OK, f"{what}: status {int(res['status'])}"
    assert (int(res["n_pieces"]), int(res["out_bytes"])) == (len(want_rows), want_bytes), what
    got_files = apply_pieces([s["open"].copy() for s in specs], pieces, bytes(out))
    for w, (got, want) in enumerate(zip(got_files, want_files)):
        assert len(got) == len(want), f"{what}: writer {w} has {len(got)} files, the referee {len(want)}"
        for k, (g, f) in enumerate(zip(got, want)):
            diff = first_diff(bytes(g.image), bytes(f.image))
            assert diff is None, f"{what}: writer {w} file {k}: {diff}"
    for j, (p, want) in enumerate(zip(pieces, want_rows)):
        got = {k: int(p[k]) for k in ROW_FIELDS}
        assert got == want, f"{what}: piece {j}: {got} != {want}"
        assert int(p["_pad"]) == 0
    return want_files


def run_case(be, rng, specs, max_count, max_size=BIG, flags=0, small=None, phases=None, gaps=False, src_phase=0,
             dst_phase=0, host_form=True, what=""):
    """Both forms against the referee; -> the referee's files."""
    writers, entries, data, batches = build_call(rng, specs, phases, gaps)
    if small is not None:
        data = force_group(entries, data, small)
    res, rows, region = device_flush(be, writers, entries, data, max_count, max_size, flags, None, None, src_phase, dst_phase)
    n, nb = int(res["n_pieces"]), int(res["out_bytes"])
    assert int(res["status"]) == OK and n <= len(entries) and nb <= len(region), f"{what}: {res}"
    assert np.all(rows[80 * n:] == 0xEE), f"{what}: piece rows behind n_pieces were written"
    assert np.all(region[nb:] == 0xEE), f"{what}: bytes behind out_bytes were written"
    assert (int(res["writer"]), int(res["entry"]), int(res["_pad"])) == (0, 0, 0), what
    pieces = rows[:80 * n].view(abi.SEG_PIECE_DTYPE)
    want_files = check_answer(specs, batches, max_count, max_size, flags, res, pieces, region[:nb], what + " (device form)")
    if host_form:
        h_p = np.full(80 * (len(entries) + 1), 0xEE, dtype=np.uint8).view(abi.SEG_PIECE_DTYPE)
        h_o = np.full(len(data) + 40 * len(entries) + 24, 0xEE, dtype=np.uint8)
        res_h, pieces_h, out_h = be.eng.segment_flush(writers, entries, data, max_count, max_size, flags, pieces=h_p, out=h_o)
        assert res_h.tobytes() == res.tobytes(), what
        assert pieces_h.tobytes() == pieces.tobytes() and out_h.tobytes() == region[:nb].tobytes(), what
        assert np.all(h_p.view(np.uint8)[80 * n:] == 0xEE) and np.all(h_o[nb:] == 0xEE), f"{what}: the host form wrote too far"
    return want_files


def n_files(want_files):
    return [len(f) for f in want_files]


# ------------------------------------------------------------------------------------------ the checks

def check_referee_worked_example():
    """The referee itself, on a case small enough to do by hand."""
    rng = np.random.default_rng(1)
    s = mk_writer(rng, [], omax=3, ocount=2, olens=[4, 6], oidx=10)
    s["entries"] = [(12, 5, b"abc"), (11, 5, b"defgh"), (20, 6, b""), (21, 6, b"zz")]
    # max_size 12: 10 bytes are there; "abc" goes in (record 2, the file's last); the file is full by count; the
    # successor takes "defgh" (0 > 12? no), "" (5 bytes) and "zz" (5 bytes): three records, MaxCount 4
    files = ref_flush([s["open"].copy()], [[(j,) + e for j, e in enumerate(s["entries"])]], 4, 12)[0]
    assert len(files) == 2 and files[0].range == (10, 12) and files[1].range == (11, 21)
    first = s["open"].image[:8 + 32 * 2] + struct.pack(">QQQII", 12, 5, 8 + 96 + 10, 3, zlib.crc32(b"abc")) + \
        s["open"].image[8 + 96:] + b"abc"
    assert bytes(files[0].image) == bytes(first)
    assert bytes(files[1].image) == python_segment([(11, 5), (20, 6), (21, 6)], [b"defgh", b"", b"zz"], 4)[:8 + 128 + 7]
    rows, total = ref_pieces([files])
    assert [(r["ordinal"], r["entry_first"], r["entry_n"], r["out_index_off"], r["out_data_off"]) for r in rows] == \
        [(0, 0, 1, 0, 32), (1, 1, 3, 43, 139)] and total == 146
    # max_size 6: the open file (10 bytes > 6) takes nothing; "abc", "defgh" (3 bytes in front of it); "" is refused
    # (8 > 6) and opens the next file with "zz" and nine bytes (2 in front of them); the last "" is refused (11 > 6)
    more = s["entries"] + [(22, 6, b"q" * 9), (23, 6, b"")]
    files = ref_flush([s["open"].copy()], [[(j,) + e for j, e in enumerate(more)]], 4, 6)[0]
    assert [f.count for f in files] == [2, 2, 3, 1] and not files[0].appended


def check_writer_sizes(be):
    """0, 1, 2, 63, 64 and 65 entries: the small-writer path and the chunked one, with boundaries of both kinds; and
    calls whose longest writer selects each sub-group width of the plan pass (8, 16, a wavefront)."""
    rng = np.random.default_rng(700)
    for sizes in ([0, 1, 2, 63, 64, 65], [0, 1, 2, 7, 8, 3], [9, 16, 0, 15, 1]):
        for max_count, max_size in ((7, BIG), (4096, 90), (5, 61)):
            specs = [mk_writer(rng, [int(x) for x in rng.integers(0, 25, size=n)], omax=6, ocount=w % 4, oidx=50 * w + 1)
                     for w, n in enumerate(sizes)]
            want = run_case(be, rng, specs, max_count, max_size, what=f"sizes {sizes} max_count {max_count} max_size {max_size}")
            assert max(n_files(want)) >= 2                    # (every call of the sweep does roll over)


def check_chunk_edges(be):
    """Writers of CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 1 entries whose file boundaries -- by count and by size --
    land on, just before and just after a chunk edge of the plan pass."""
    rng = np.random.default_rng(710)
    sizes = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
    for k in (CHUNK - 1, CHUNK, CHUNK + 1):
        # by count: k records of room in the open file, then successors of k records
        specs = [mk_writer(rng, [int(x) for x in rng.integers(0, 9, size=n)], omax=k + 2, ocount=2) for n in sizes]
        want = run_case(be, rng, specs, k, what=f"count boundary every {k}")
        assert n_files(want) == [1 + (n > k) + (n > 2 * k) for n in sizes]
        # by size: 10-byte payloads and max_size 10 k - 1: a file is full once it holds k entries
        specs = [mk_writer(rng, [10] * n, omax=4096) for n in sizes]
        want = run_case(be, rng, specs, 4096, 10 * k - 1, what=f"size boundary every {k}")
        assert n_files(want) == [(n + k - 1) // k for n in sizes]
        # both, out of step: the size limit inside the first chunk, the count limit behind the edge
        specs = [mk_writer(rng, [10] * n, omax=4096, ocount=3, olens=[10, 10, 10]) for n in sizes]
        run_case(be, rng, specs, k - 5, 10 * 40 - 1, what=f"size 40, count {k - 5}")


def check_small_max_counts(be):
    rng = np.random.default_rng(720)
    for max_count in (1, 2, 3):
        sizes = sorted({max(0, k * max_count + d) for k in (1, 2, 5) for d in (-1, 0, 1)})
        for omax, ocount in ((max_count, 0), (max_count, max_count), (4, 3), (4, 4), (9, 2)):
            specs = [mk_writer(rng, [int(x) for x in rng.integers(0, 20, size=n)], omax=omax, ocount=ocount) for n in sizes]
            want = run_case(be, rng, specs, max_count, what=f"max_count {max_count} open {ocount}/{omax}")
            room = omax - ocount
            assert n_files(want) == [1 + (max(0, n - room) + max_count - 1) // max_count for n in sizes]
            if ocount == omax:                               # an open segment that is full already: no ordinal-0 piece
                assert all(not f[0].appended for f in want)


def check_open_states(be):
    """open_count = open_max_count and one below; open_max_count != max_count; open_data_bytes = max_size (not full)
    and max_size + 1 (full)."""
    rng = np.random.default_rng(730)
    lens = [7, 0, 9, 30, 2, 2, 11]
    for max_size, olens in ((40, [20, 20]), (40, [20, 21]), (41, [20, 21]), (0, []), (0, [1])):
        specs = [mk_writer(rng, lens, omax=om, ocount=len(olens), olens=olens) for om in (len(olens) or 1, len(olens) + 1, 50)]
        want = run_case(be, rng, specs, 3, max_size, what=f"open bytes {sum(olens)} max_size {max_size}")
        full = sum(olens) > max_size
        assert [bool(f[0].appended) for f in want] == [False if full else len(olens) < om for om in (len(olens) or 1, len(olens) + 1, 50)]
    specs = [mk_writer(rng, lens, omax=om, ocount=oc) for om, oc in ((5, 5), (5, 4), (2, 0), (65535, 65535 - 3))]
    specs[3] = mk_writer(rng, lens, omax=65535, ocount=3)       # (a 65535-record open file costs 2 MiB: keep it at 3)
    want = run_case(be, rng, specs, 4, what="open counts")
    assert n_files(want) == [3, 3, 3, 1]


def check_payload_edges(be):
    rng = np.random.default_rng(740)
    # zero-length payloads, a run of them across a count boundary and behind a size boundary
    specs = [mk_writer(rng, [0] * 9, omax=4, ocount=1), mk_writer(rng, [5, 0, 0, 0, 0, 6, 0, 0], omax=3),
             mk_writer(rng, [0, 0, 50, 0, 0, 0, 1, 0], omax=8), mk_writer(rng, [0], omax=1, ocount=1)]
    want = run_case(be, rng, specs, 3, 40, what="zero-length payloads")
    assert n_files(want) == [3, 3, 3, 2]
    # one payload longer than max_size on its own: it goes in (the test comes first), its successor does not
    specs = [mk_writer(rng, [500]), mk_writer(rng, [3, 500, 3, 3]), mk_writer(rng, [500, 500, 500], ocount=2, olens=[50, 50])]
    want = run_case(be, rng, specs, 100, 99, what="payload > max_size")
    assert n_files(want) == [1, 2, 4]
    # indexes that go backwards inside a writer and below the open range: {min, last}
    specs = [mk_writer(rng, [4] * 6, omax=4, ocount=2, oidx=100, idxs=[102, 103, 90, 91, 50, 51]),
             mk_writer(rng, [4] * 5, omax=50, ocount=3, oidx=100, idxs=[103, 7, 8, 9, 8]),
             mk_writer(rng, [4] * 3, omax=50, idxs=[30, 20, 25])]
    want = run_case(be, rng, specs, 3, what="backwards indexes")
    assert [f.range for f in want[0]] == [(100, 103), (50, 50), (51, 51)]      # 90, 91, 50 share a file: {50, 50}
    assert want[1][0].range == (7, 8) and want[2][0].range == (20, 25)
    # index and term across 2^32 and 2^63
    wide = [(1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 2, 5]
    specs = [mk_writer(rng, [6] * 6, omax=4, ocount=1, oidx=(1 << 32) - 2, idxs=wide, terms=wide[::-1])]
    run_case(be, rng, specs, 2, what="wide index and term")
    # open_data_bytes beyond 2^32 with a large max_size: a 64-bit DataOffset, no data needed at that offset
    for hole in ((1 << 32) + 12345, (1 << 45) + 1):
        specs = [mk_writer(rng, [9, 0, 30, 4], omax=16, ocount=2, olens=[3, 4], hole=hole), mk_writer(rng, [5, 5])]
        want = run_case(be, rng, specs, 3, 1 << 50, what=f"open_data_bytes 7 + {hole}")
        assert n_files(want) == [1, 1] and want[0][0].data_offset == 8 + 32 * 16 + 7 + hole + 43
        want = run_case(be, rng, specs, 3, hole, what=f"open_data_bytes 7 + {hole}, full")       # 7 + hole > hole
        assert n_files(want) == [3, 1] and not want[0][0].appended


def check_every_length_and_phase(be, small):
    """Payload lengths 0..80 and those around 16 GROUP at every source phase; the whole answer at several destination
    phases (all sixteen on the GPU) -- consecutive payloads of odd lengths put the copies at every phase as well."""
    rng = np.random.default_rng(750 + small)
    lens = ([1007, 1008, 1023, 1024, 1025, 1040, 2049], [255, 256, 257, 272, 511, 513], [127, 128, 129, 240])[small]
    lens = lens + (list(range(81)) if small == 2 or be.gpu else list(range(0, 81, 5)))
    flat = [(ln, sp) for ln in lens for sp in range(16)]
    cut = len(flat) // 3
    # three writers: a fresh open file, one that rolls over by count in the middle, one with a size limit
    specs = [mk_writer(rng, [f[0] for f in flat[:cut]], omax=4096), mk_writer(rng, [f[0] for f in flat[cut:2 * cut]], omax=40, ocount=3),
             mk_writer(rng, [f[0] for f in flat[2 * cut:]], omax=4096, ocount=1, olens=[11])]
    writers, entries, data, batches = build_call(rng, specs, [f[1] for f in flat])
    data = force_group(entries, data, small)
    for flags in (0, NO_CRC):
        for dp in ((0, 1, 7, 8, 15) if not be.gpu else range(16)):
            if flags and dp not in (0, 7):
                continue
            res, rows, region = device_flush(be, writers, entries, data, 500, 30000, flags, None, None, (dp * 5) % 16, dp)
            n, nb = int(res["n_pieces"]), int(res["out_bytes"])
            assert int(res["status"]) == OK and np.all(rows[80 * n:] == 0xEE) and np.all(region[nb:] == 0xEE)
            want = check_answer(specs, batches, 500, 30000, flags, res, rows[:80 * n].view(abi.SEG_PIECE_DTYPE), region[:nb],
                                f"width {small} flags {flags} destination phase {dp}")
            assert max(n_files(want)) >= 2
    seen = set()
    for p in rows[:80 * n].view(abi.SEG_PIECE_DTYPE):
        pos = int(p["out_data_off"])
        for e in range(int(p["entry_first"]), int(p["entry_first"]) + int(p["entry_n"])):
            seen.add(pos % 16); pos += int(entries["data_len"][e])
    assert len(seen) == 16, "the sweep misses a destination phase"


def check_against_build_and_read_back(be):
    """A fresh writer whose entries fit: header + index piece + zero fill + data piece is the rgb_segment_build image of
    the same entries.  And rgb_segment_scan / rgb_segment_info read every produced file back with the referee's counts
    and range."""
    rng = np.random.default_rng(760)
    for n, mc in ((1, 1), (5, 9), (40, 40)):
        specs = [mk_writer(rng, [int(x) for x in rng.integers(0, 300, size=n)], omax=mc)]
        writers, entries, data, batches = build_call(rng, specs)
        res, pieces, out = be.eng.segment_flush(writers, entries, data, mc)
        assert int(res["status"]) == OK and len(pieces) == 1
        p = pieces[0]
        io, do, db = int(p["out_index_off"]), int(p["out_data_off"]), int(p["data_bytes"])
        assert (int(p["index_file_off"]), int(p["data_file_off"])) == (8, 8 + 32 * mc)
        image = struct.pack(">4sHH", b"RASG", 2, mc) + out[io:io + 32 * n].tobytes() + bytes(32 * (mc - n)) + out[do:do + db].tobytes()
        assert first_diff(image, be.eng.segment_build(entries, data, mc).tobytes()) is None, (n, mc)
    specs = [mk_writer(rng, [int(x) for x in rng.integers(0, 60, size=n)], omax=6, ocount=w % 3, oidx=1000 * w + 9)
             for w, n in enumerate((0, 3, 11, 30, 70))]
    specs[2]["entries"][4] = (5, 9, b"low index")
    want = run_case(be, rng, specs, 8, 300, what="read back")
    files = [f for lst in want for f in lst]
    images = [bytes(f.image) + bytes(max(0, f.data_start - len(f.image))) for f in files]
    sources = np.zeros(len(files), dtype=abi.SEG_SOURCE_DTYPE)
    sources["n_bytes"] = [len(i) for i in images]
    sources["offset"] = np.cumsum([0] + [len(i) for i in images[:-1]])
    infos = be.eng.segment_info(sources, np.frombuffer(b"".join(images), dtype=np.uint8), None)
    for f, image, info in zip(files, images, infos):
        recs, version, max_count, end = be.engine.segment_scan(image)
        assert (len(recs), version, max_count) == (f.count, 2, f.max_count)
        assert end == (abi.SEG_END_FULL if f.count == f.max_count else abi.SEG_END_ZEROS)
        assert be.eng.segment_validate(np.frombuffer(image, dtype=np.uint8), recs) == f.count
        assert (int(info["num_entries"]), int(info["max_count"])) == (f.count, f.max_count)
        if f.count:
            assert (int(info["range_first"]), int(info["range_last"])) == f.range


def malformed_writers():
    """(name, rows of (entry_first, entry_n, open_count, open_max_count, open_data_bytes, range_first, range_last),
    n_entries) -- each is RGB_E_INVAL"""
    U = UNDEF
    good = (0, 4, 0, 8, 0, U, U)
    return [("slice outside the entries", [(8, 3, 0, 8, 0, U, U)], 10),
            ("slice start outside the entries", [(11, 0, 0, 8, 0, U, U)], 10),
            ("slice wraps", [(0xFFFFFFFF, 2, 0, 8, 0, U, U)], 10),
            ("not ascending", [(4, 2, 0, 8, 0, U, U), (0, 2, 0, 8, 0, U, U)], 10),
            ("overlapping", [good, (3, 2, 0, 8, 0, U, U)], 10),
            ("open_max_count 0", [(0, 4, 0, 0, 0, U, U)], 10),
            ("open_max_count 65536", [(0, 4, 0, 65536, 0, U, U)], 10),
            ("open_count > open_max_count", [(0, 4, 9, 8, 0, 1, 9)], 10),
            ("a range without records", [(0, 4, 0, 8, 0, 1, 2)], 10),
            ("half a range", [(0, 4, 0, 8, 0, U, 2)], 10),
            ("records without a range", [(0, 4, 2, 8, 0, U, U)], 10),
            ("records with half a range", [(0, 4, 2, 8, 0, 3, U)], 10),
            ("range_first > range_last", [(0, 4, 2, 8, 0, 6, 5)], 10),
            ("the second writer", [good, (4, 2, 2, 8, 0, 6, 5)], 10)]


def rows_to_writers(rows):
    w = np.zeros(len(rows), dtype=abi.SEG_WRITER_DTYPE)
    for i, r in enumerate(rows):
        w[i] = tuple(r) + (0,)
    return w


def check_statuses_and_errors(be):
    rng = np.random.default_rng(770)
    specs = [mk_writer(rng, [int(x) for x in rng.integers(0, 40, size=n)], omax=5, ocount=w % 3, oidx=100 * w + 1)
             for w, n in enumerate((4, 0, 9, 17))]
    writers, entries, data, batches = build_call(rng, specs)
    want_rows, want_bytes = ref_pieces(ref_flush([s["open"].copy() for s in specs], batches, 4, 100))
    assert len(want_rows) > 6

    def untouched(rows, region):
        return np.all(rows == 0xEE) and np.all(region == 0xEE)

    # SPACE: one byte or one row short; what is needed is reported, nothing is written
    for cap, room in ((len(want_rows), want_bytes - 1), (len(want_rows) - 1, want_bytes), (0, 0)):
        res, rows, region = device_flush(be, writers, entries, data, 4, 100, 0, cap, room)
        assert (int(res["status"]), int(res["n_pieces"]), int(res["out_bytes"])) == (SPACE, len(want_rows), want_bytes)
        assert untouched(rows, region)
        h_p, h_o = np.full(80 * cap, 0xEE, dtype=np.uint8).view(abi.SEG_PIECE_DTYPE), np.full(room, 0xEE, dtype=np.uint8)
        res_h, pieces_h, out_h = be.eng.segment_flush(writers, entries, data, 4, 100, 0, pieces=h_p, out=h_o)
        assert res_h.tobytes() == res.tobytes() and pieces_h is None and out_h is None
        assert untouched(h_p.view(np.uint8), h_o)
    res, rows, region = device_flush(be, writers, entries, data, 4, 100, 0, len(want_rows), want_bytes)        # exactly enough
    assert (int(res["status"]), int(res["n_pieces"]), int(res["out_bytes"])) == (OK, len(want_rows), want_bytes)

    # ENTRY: the first entry, in entry order, whose payload lies outside d_data -- RGB_E_INVAL on the host-buffer form
    for bad_at, field, value in (((7, 22), "data_len", len(data)), ((22, 7), "data_offset", (1 << 64) - 4),
                                 ((29,), "data_offset", len(data) + 1), ((0, 29), "data_len", len(data) + 1)):
        bad = entries.copy()
        for e in bad_at:
            bad[field][e] = value
        first = min(bad_at)
        res, rows, region = device_flush(be, writers, bad, data, 4, 100)
        assert (int(res["status"]), int(res["entry"])) == (ENTRY, first), bad_at
        assert int(res["writer"]) == max(w for w in range(len(writers)) if int(writers["entry_first"][w]) <= first and
                                         int(writers["entry_n"][w])), bad_at
        assert untouched(rows, region)
        res, rows, region = device_flush(be, writers, bad, data, 4, 100, 0, 0, 0)                  # ENTRY is looked at before SPACE
        assert int(res["status"]) == ENTRY
        h_o = np.full(want_bytes + 50, 0xEE, dtype=np.uint8)
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.segment_flush(writers, bad, data, 4, 100, out=h_o)
        assert e.value.code == E_INVAL and np.all(h_o == 0xEE)
    # a payload that ends exactly at the end of the data is inside; an entry of no writer may point anywhere
    edge = entries.copy()
    edge["data_offset"][3], edge["data_len"][3] = len(data) - 10, 10
    assert int(device_flush(be, writers, edge, data, 4, 100)[0]["status"]) == OK
    loose = np.concatenate([entries, entries[:1]])
    loose["data_offset"][-1] = 1 << 60
    res, rows, region = device_flush(be, writers, loose, data, 4, 100)
    assert (int(res["status"]), int(res["n_pieces"]), int(res["out_bytes"])) == (OK, len(want_rows), want_bytes)

    # descriptor faults, limits of max_count, unknown flags: RGB_E_INVAL with nothing written
    calls = [(name, rows_to_writers(rows), n_e, 4, 0) for name, rows, n_e in malformed_writers()]
    calls += [("max_count 0", writers, len(entries), 0, 0), ("max_count 65536", writers, len(entries), 65536, 0),
              ("unknown flags", writers, len(entries), 4, 2), ("unknown flags", writers, len(entries), 4, 1 << 31)]
    for name, wr, n_e, max_count, flags in calls:
        ents = np.zeros(n_e, dtype=abi.SEG_ENTRY_DTYPE) if wr is not writers else entries
        if wr is not writers:
            with pytest.raises(be.engine.RgbError) as e:
                be.engine.segment_flush_bound(wr, n_e, 100)
            assert e.value.code == E_INVAL, name
        h_p, h_o = np.full(800, 0xEE, dtype=np.uint8).view(abi.SEG_PIECE_DTYPE), np.full(4000, 0xEE, dtype=np.uint8)
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.segment_flush(wr, ents, data, max_count, 100, flags, pieces=h_p, out=h_o)
        assert e.value.code == E_INVAL and untouched(h_p.view(np.uint8), h_o), name
        d_o, p_o, b_o = be.dev(np.full(4000 + 800 + 32, 0xEE, dtype=np.uint8))
        d_e, p_e, _ = be.dev(ents.view(np.uint8))
        d_d, p_d, _ = be.dev(data)
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.segment_flush_device(wr, p_e, n_e, p_d, len(data), p_o + 4000, 10, p_o, 4000, p_o + 4800, max_count, 100, flags)
        assert e.value.code == E_INVAL, name
        assert np.all(be.get(d_o)[b_o:b_o + 4832] == 0xEE), f"{name}: refused, but something was written"
    # the limits themselves are legal
    assert be.engine.segment_flush_bound(rows_to_writers([(0, 10, 65535, 65535, 1 << 62, 0, UNDEF - 1)]), 10, 7) == (407, 10)

    # empty calls: no writers, no entries, writers without entries
    none = np.zeros(0, dtype=abi.SEG_WRITER_DTYPE)
    for wr, ents, dat in ((none, entries[:0], data[:0]), (none, entries, data),
                          (rows_to_writers([(0, 0, 0, 8, 0, UNDEF, UNDEF), (3, 0, 2, 2, 9, 1, 2)]), entries, data)):
        res, rows, region = device_flush(be, wr, ents, dat, 4, 100)
        assert (int(res["status"]), int(res["n_pieces"]), int(res["out_bytes"])) == (OK, 0, 0) and untouched(rows, region)
        res_h, pieces_h, out_h = be.eng.segment_flush(wr, ents, dat, 4, 100)
        assert int(res_h["status"]) == OK and len(pieces_h) == 0 and len(out_h) == 0


def check_spread_bad_entries(be):
    """ENTRY names the first entry, in entry order, whose payload lies outside d_data: a 64-bit minimum over atomics
    (s_bad of the plan pass, then over the workgroups' totals in the place pass) that arrive in whatever order lanes and
    workgroups run.  Three bad entries far apart -- two in one workgroup of the plan on different wavefronts, the third
    more than 256 entries on in another workgroup -- at both ends of the sub-group widths; the same calls without the
    damage go against the referee."""
    rng = np.random.default_rng(775)
    for n_writers, per, bad_at in ((12, 30, (300, 50, 20)),        # a wavefront per writer: 4 writers, 3 workgroups
                                   (100, 4, (330, 200, 40))):      # 8 lanes per writer: 32 writers, 4 workgroups
        specs = [mk_writer(rng, [int(x) for x in rng.integers(0, 20, size=per)], omax=5, ocount=w % 3, oidx=100 * w + 1)
                 for w in range(n_writers)]
        what = f"{n_writers} writers of {per} entries"
        run_case(be, rng, specs, 4, 100, host_form=False, what=what)
        writers, entries, data, _ = build_call(rng, specs)
        assert len(entries) == n_writers * per and max(bad_at) - min(bad_at) > 256
        for field, value in (("data_len", len(data) + 1), ("data_offset", (1 << 64) - 4)):
            bad = entries.copy()
            for e in bad_at:
                bad[field][e] = value
            res, rows, region = device_flush(be, writers, bad, data, 4, 100)
            got = (int(res["status"]), int(res["entry"]), int(res["writer"]))
            assert got == (ENTRY, min(bad_at), min(bad_at) // per), f"{what}, {field} of {bad_at}: {got}"
            assert np.all(rows == 0xEE) and np.all(region == 0xEE), f"{what}: ENTRY, but something was written"


def random_specs(rng, trial):
    n_w = int(rng.integers(0, 6))
    long_one = trial % 7 == 0
    max_count = int(rng.choice([1, 2, 3, 5, 8, 40, 4096]))
    max_size = int(rng.choice([0, 1, 30, 64, 200, 1000, BIG]))
    specs = []
    for w in range(n_w):
        n = int(rng.integers(0, 13)) if not (long_one and w == 0) else int(rng.integers(CHUNK - 2, 2 * CHUNK + 3))
        omax = int(rng.choice([1, 2, 6, 70, 65535 if w == 1 else 9]))
        ocount = int(rng.integers(0, min(omax, 5) + 1)) if omax < 65535 else 3
        if rng.random() < 0.2:
            ocount = min(omax, 6)
        olens = [int(x) for x in rng.integers(0, 40, size=ocount)]
        hole = int(rng.choice([0, 0, 0, (1 << 32) + 5, 1 << 50]))
        lens = [int(x) for x in rng.choice([0, 0, 1, 7, 15, 16, 17, 33, 40, 300], size=n)]
        oidx = int(rng.choice([1, 1000, (1 << 32) - 3, (1 << 63) - 2]))
        idxs = None
        if rng.random() < 0.4:
            idxs = [(oidx if oidx > 1 else 1) + int(x) for x in rng.integers(-1, 12, size=n)]
        specs.append(mk_writer(rng, lens, omax, ocount, olens, hole if max_size == BIG or hole == 0 else 0, oidx, idxs,
                               [int(x) for x in rng.integers(0, 1 << 63, size=n, dtype=np.uint64)]))
    return specs, max_count, (max_size if max_size != BIG else (1 << 63))


def check_random_sweep(be, first, count):
    for trial in range(first, first + count):
        rng = np.random.default_rng(8000 + trial)
        specs, max_count, max_size = random_specs(rng, trial)
        run_case(be, rng, specs, max_count, max_size, flags=NO_CRC if trial % 5 == 0 else 0, gaps=trial % 3 == 0,
                 small=2 if trial % 4 else None, src_phase=trial % 16, dst_phase=(trial * 7) % 16, host_form=trial % 3 == 1,
                 what=f"trial {trial}")


def check_back_to_back_calls(be):
    """Two calls of the device form on a fresh context with nothing waited for in between.  The first (one writer, one
    entry) leaves a pinned block of 128 bytes for the writers and a device copy of 4192; the second has 128 writers at
    48 bytes each, so both blocks are regrown while the first call's upload and kernels may still be under way.  Only
    the GPU half has anything in flight: the emulation runs each call to its end, and there this checks the regrowth
    alone.  The sizes are those of rgb_segment.hip's growth rules (pinned: twice the need; device: need + need / 2 +
    4096) worked out by hand; the library does not report its capacities, so the assertion below documents the shapes
    and does not follow a change of those rules."""
    rng = np.random.default_rng(790)
    calls = []
    for n_writers in (1, 128):
        specs = [mk_writer(rng, [int(rng.integers(0, 40))], omax=4, ocount=w % 3, oidx=10 * w + 1) for w in range(n_writers)]
        calls.append((specs,) + build_call(rng, specs))
    assert 48 * len(calls[1][0]) > max(128, 4192)
    fresh = type(be)(be.engine)
    try:
        runs = [prepared_flush(fresh, writers, entries, data, 3, BIG) for _, writers, entries, data, _ in calls]
        for call, _ in runs:
            call()
        for (specs, _, _, _, batches), (_, fetch) in zip(calls, runs):
            res, rows, region = fetch()
            n, nb = int(res["n_pieces"]), int(res["out_bytes"])
            check_answer(specs, batches, 3, BIG, 0, res, rows[:80 * n].view(abi.SEG_PIECE_DTYPE), region[:nb],
                         f"{len(specs)} writers")
            assert np.all(rows[80 * n:] == 0xEE) and np.all(region[nb:] == 0xEE), "wrote behind the answer"
    finally:
        fresh.close()


def check_many_writers(be):
    """65 536 writers x 3 entries of 40..200 bytes with mixed open states, one call, against the referee."""
    rng = np.random.default_rng(780)
    n_w = 65536
    blob = rnd_bytes(rng, 1 << 16)
    specs = []
    for w in range(n_w):
        omax, ocount = ((4, 0), (4, 2), (4, 3), (4, 4), (9, 8), (2, 1), (300, 7), (3, 0))[w % 8]
        olens = [5] * ocount
        image = python_segment([(10 + j, 1) for j in range(ocount)], [blob[j:j + 5] for j in range(ocount)], omax)
        lens = rng.integers(40, 201, size=3)
        off = int(rng.integers(0, len(blob) - 700))
        ents, pos = [], off
        for j, ln in enumerate(lens):
            ents.append((10 + ocount + j if w % 16 else 12 - j, 3, blob[pos:pos + int(ln)])); pos += int(ln)
        specs.append(dict(open=RefFile(omax, image, ocount, 5 * ocount, (10, 9 + ocount) if ocount else None), entries=ents))
    want = run_case(be, rng, specs, 2, 230, host_form=False, what="65536 writers")
    assert len(set(n_files(want))) >= 3


# ------------------------------------------------------------------------------------------ CPU (emulation)

def test_abi_mirror():
    hdr = " ".join(open(os.path.join(ROOT, "include", "ra_gpu_wal.h")).read().split())
    for name, val in (("RGB_SEG_FLUSH_OK", abi.SEG_FLUSH_OK), ("RGB_SEG_FLUSH_SPACE", abi.SEG_FLUSH_SPACE),
                      ("RGB_SEG_FLUSH_ENTRY", abi.SEG_FLUSH_ENTRY)):
        assert int(hdr.split(f"#define {name} ")[1].split()[0].rstrip("u")) == val, name
    assert (OK, SPACE, ENTRY) == (abi.SEG_FLUSH_OK, abi.SEG_FLUSH_SPACE, abi.SEG_FLUSH_ENTRY)
    assert "#define RGB_ABI_VERSION 10u" in " ".join(open(os.path.join(ROOT, "include", "ra_gpu_batch.h")).read().split())
    assert (abi.SEG_WRITER_DTYPE.itemsize, abi.SEG_PIECE_DTYPE.itemsize, abi.SEG_FLUSH_RESULT_DTYPE.itemsize) == (48, 80, 32)
    assert abi.SEG_WRITER_DTYPE.fields["open_data_bytes"][1] == 16 and abi.SEG_WRITER_DTYPE.fields["range_last"][1] == 32
    assert abi.SEG_PIECE_DTYPE.fields["out_index_off"][1] == 32 and abi.SEG_PIECE_DTYPE.fields["max_count"][1] == 72
    assert abi.SEG_FLUSH_RESULT_DTYPE.fields["out_bytes"][1] == 8 and abi.SEG_FLUSH_RESULT_DTYPE.fields["entry"][1] == 20
    assert CHUNK == int(open(os.path.join(ROOT, "ra_amd", "csrc", "rgb_segment.hip")).read().split("FL_CHUNK = ")[1].split(";")[0])


def test_referee_on_a_worked_example():
    check_referee_worked_example()


def test_emu_writer_sizes(emu):
    check_writer_sizes(emu)


def test_emu_chunk_edges(emu):
    check_chunk_edges(emu)


def test_emu_small_max_counts(emu):
    check_small_max_counts(emu)


def test_emu_open_states(emu):
    check_open_states(emu)


def test_emu_payload_edges(emu):
    check_payload_edges(emu)


@pytest.mark.parametrize("small", [0, 1, 2], ids=["wave_per_entry", "four_per_wave", "eight_per_wave"])
def test_emu_every_length_and_phase(emu, small):
    check_every_length_and_phase(emu, small)


def test_emu_against_build_and_read_back(emu):
    check_against_build_and_read_back(emu)


def test_emu_statuses_and_errors(emu):
    check_statuses_and_errors(emu)


@pytest.mark.parametrize("first", [0, 100, 200])
def test_emu_random_sweep(emu, first):
    check_random_sweep(emu, first, 100)


def test_emu_back_to_back_calls(emu):
    check_back_to_back_calls(emu)


def test_emu_spread_bad_entries(emu):
    check_spread_bad_entries(emu)


@pytest.mark.parametrize("sched", PERMUTED_SCHEDULES)
def test_emu_under_permuted_schedules(emu, sched):
    """The emulation's own order is workgroups 0, 1, 2, ... and lanes 0 .. 255, so the first bad entry also arrives
    first at the minimum that finds it, and every workgroup of the place pass runs behind its predecessors.  The checks
    that span several workgroups once more with workgroups and lanes reversed and permuted (tests/emu_schedule.py);
    the referee stays ref_flush."""
    with schedule(emu.engine, sched):
        check_chunk_edges(emu)
        check_statuses_and_errors(emu)
        check_spread_bad_entries(emu)
        check_random_sweep(emu, 100, 40)


def test_flush_descriptors_under_sanitizers(tmp_path):
    """rgb_segment_flush_bound -- the host-side validation of every flush call, in the host-only unit
    rgb_segment_host.cpp -- compiled with AddressSanitizer + UBSan into a stand-alone program and run over the malformed
    writers of check_statuses_and_errors and some good ones, each array in an exactly-sized heap block."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "segment_flush_harness"
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-o", str(exe),
           os.path.join(ROOT, "tests", "native", "segment_flush_harness.cpp"),
           os.path.join(ROOT, "ra_amd", "csrc", "rgb_segment_host.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert built.returncode == 0, built.stderr
    cases = [(rows_to_writers(rows), n_e, 100, E_INVAL, 0, 0) for _, rows, n_e in malformed_writers()]
    U = UNDEF
    good = rows_to_writers([(0, 3, 0, 1, 0, U, U), (3, 0, 65535, 65535, 1 << 40, 0, U - 1), (5, 5, 1, 2, 0, 7, 7)])
    cases.append((good, 10, 1000, 0, 1000 + 400, 10))
    cases.append((good[:0], 0, 0, 0, 0, 0))
    cases.append((good[:0], 0xFFFFFFFF, 1 << 40, 0, (1 << 40) + 40 * 0xFFFFFFFF, 0xFFFFFFFF))
    cases.append((good[:1], 3, UNDEF - 100, E_INVAL, 0, 0))                  # the bound itself would wrap
    files = []
    for k, (w, n_e, db, _, _, _) in enumerate(cases):
        path = tmp_path / f"w{k}.bin"
        path.write_bytes(struct.pack("<IIQ", len(w), n_e, db) + w.tobytes())
        files.append(str(path))
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in run.stdout.splitlines()]
    assert got == [c[3:] for c in cases]


def test_flush_kernels_use_no_scratch():
    """hipcc's resource remarks for gfx950 (no GPU needed), as tests/test_kernel_resources.py reads them: the kernels
    of the three passes without scratch or spills; the copy's occupancy and LDS size no worse than those of
    rgb_seg_crc_kernel<GROUP, true> of the same width at the commit before (PARENT_BUILD_KERNELS)."""
    from test_kernel_resources import segment_usage
    usage = segment_usage()
    names = [k for k in usage if "rgb_flush_" in k]
    assert len(names) == 7, names                       # 3 widths of plan, place, 3 widths of copy
    for k in names:
        u = usage[k]
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, f"{k}: {u}"
    for group, (occupancy, lds) in PARENT_BUILD_KERNELS.items():
        (k,) = [k for k in names if f"rgb_flush_copy_kernelILi{group}E" in k]
        assert usage[k]["Occupancy"] >= occupancy and usage[k]["LDS Size"] <= lds, f"{k}: {usage[k]}"
        (b,) = [b for b in usage if f"rgb_seg_crc_kernelILi{group}ELb1E" in b]              # unchanged by this feature
        assert (usage[b]["Occupancy"], usage[b]["LDS Size"]) == (occupancy, lds), f"{b}: {usage[b]}"


# ------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
def test_gpu_writer_sizes(gpu):
    check_writer_sizes(gpu)


@pytest.mark.gpu
def test_gpu_chunk_edges(gpu):
    check_chunk_edges(gpu)


@pytest.mark.gpu
def test_gpu_small_max_counts(gpu):
    check_small_max_counts(gpu)


@pytest.mark.gpu
def test_gpu_open_states(gpu):
    check_open_states(gpu)


@pytest.mark.gpu
def test_gpu_payload_edges(gpu):
    check_payload_edges(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("small", [0, 1, 2], ids=["wave_per_entry", "four_per_wave", "eight_per_wave"])
def test_gpu_every_length_and_phase(gpu, small):
    check_every_length_and_phase(gpu, small)


@pytest.mark.gpu
def test_gpu_against_build_and_read_back(gpu):
    check_against_build_and_read_back(gpu)


@pytest.mark.gpu
def test_gpu_statuses_and_errors(gpu):
    check_statuses_and_errors(gpu)


@pytest.mark.gpu
def test_gpu_random_sweep(gpu):
    check_random_sweep(gpu, 0, 300)


@pytest.mark.gpu
def test_gpu_back_to_back_calls(gpu):
    check_back_to_back_calls(gpu)


@pytest.mark.gpu
def test_gpu_spread_bad_entries(gpu):
    check_spread_bad_entries(gpu)


@pytest.mark.gpu
def test_gpu_many_writers(gpu):
    """GPU only: the emulation runs the plan of 65 536 writers and the copy of 196 608 entries lane by lane, far beyond
    the few seconds a test may cost."""
    check_many_writers(gpu)
