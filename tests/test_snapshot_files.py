"""Snapshot files on the device: ragged CRC batches, snapshot.dat / indexes images and their validation
(include/ra_gpu_wal.h, "snapshots and checkpoints"; ra_amd/csrc/rgb_segment.hip, rgb_segment_host.cpp).

Referee: struct.pack and zlib.crc32 -- the function erlang:crc32 is -- over the formats as the reference source states them:
  src/ra_log_snapshot.erl:49-68     write/4: <<"RASN", 1:8, Crc:32>>, Data = [<<MetaSize:32>>, Meta | IOVec], Crc = crc32(Data)
  src/ra_log_snapshot.erl:104-108   accept_chunk/2: erlang:crc32(PartialCrc0, Chunk)
  src/ra_log_snapshot.erl:176-187   recover/1: version 1 -> validate; other version -> {invalid_version, V}; else invalid_format
  src/ra_log_snapshot.erl:234-253   read_meta_internal/1: 13 bytes read; eof; the second clause needs 9 bytes only
  src/ra_log_snapshot.erl:255-266   validate/2: crc32(Data) =:= Crc or checksum_error; parse_snapshot/1
  src/ra_snapshot.erl:1017-1059     write_indexes/2, indexes/1: <<"RASI", 1:8, Crc:32, Data/binary>>, Crc = crc32(Data)
There is no OTP here, so no file written by the reference itself can be a fixture; the images are packed by hand.

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
from test_segment import (E_INVAL, ROOT, STREAM_BLOCK, emu, first_diff, gf2_mulmod, gf2_xpow8, gpu,  # noqa: F401
                          raw_crc)

B = STREAM_BLOCK               # rgb_segment.hip: SNAP_BLOCK, the bytes of a long piece per workgroup step
TIERS = (321, 1024, 16384)     # ... and the first length of the 16-lane, 64-lane and block passes (SNAP_T8 + 1, SNAP_T16, SNAP_TBLOCK)
SNAPSHOT, INDEXES = abi.SNAP_KIND_SNAPSHOT, abi.SNAP_KIND_INDEXES
GUARD = 32                     # poisoned bytes on either side of every output


# ------------------------------------------------------------------------------------------ referee

def ref_image(kind, meta: bytes, data: bytes) -> bytes:
    if kind == SNAPSHOT:
        body = struct.pack(">I", len(meta)) + meta + data
        return struct.pack(">4sBI", b"RASN", 1, zlib.crc32(body)) + body
    return struct.pack(">4sBI", b"RASI", 1, zlib.crc32(data)) + data


def ref_info(buf: bytes, off: int, n: int, kind: int, meta_only: bool):
    """(status, version, stored_crc, computed_crc, meta_offset, meta_len, data_offset, data_bytes) of one file"""
    f = buf[off:off + n]
    magic = b"RASN" if kind == SNAPSHOT else b"RASI"
    if meta_only and n == 0:
        return (abi.SNAP_EOF, 0, 0, 0, 0, 0, 0, 0)                     # eof -> unexpected_eof_when_parsing_header
    if n < 9 or f[:4] != magic:
        return (abi.SNAP_INVALID_FORMAT, 0, 0, 0, 0, 0, 0, 0)
    version, stored = f[4], struct.unpack(">I", f[5:9])[0]
    if version != 1 or (meta_only and kind == SNAPSHOT and n < 13):    # read_meta_internal's second clause
        return (abi.SNAP_INVALID_VERSION, version, stored, 0, 0, 0, 0, 0)
    crc = 0
    if not meta_only:
        crc = zlib.crc32(f[9:])
        if crc != stored:
            return (abi.SNAP_CHECKSUM, 1, stored, crc, 0, 0, 0, 0)
    if kind == INDEXES:
        return (abi.SNAP_OK, 1, stored, crc, 0, 0, off + 9, n - 9)
    if n < 13 or struct.unpack(">I", f[9:13])[0] > n - 13:             # parse_snapshot/1 has no clause / the short read
        return (abi.SNAP_BAD_META, 1, stored, crc, 0, 0, 0, 0)
    ms = struct.unpack(">I", f[9:13])[0]
    return (abi.SNAP_OK, 1, stored, crc, off + 13, ms, off + 13 + ms, n - 13 - ms)


INFO_FIELDS = ("status", "version", "stored_crc", "computed_crc", "meta_offset", "meta_len", "data_offset", "data_bytes")


def rows_as_tuples(infos):
    return [tuple(int(r[f]) for f in INFO_FIELDS) for r in infos]


# ------------------------------------------------------------------------------------------ through the library

def guarded(be, n_bytes, phase=0):
    """A poisoned device output of n_bytes between GUARD poisoned bytes -> (buffer, pointer, read())"""
    d, p, b = be.dev(np.full(n_bytes + 2 * GUARD, 0xEE, dtype=np.uint8), phase)

    def read():
        got = be.get(d)
        assert np.all(got[:b] == 0) and np.all(got[b + n_bytes + 2 * GUARD:] == 0), "wrote outside the buffer"
        assert np.all(got[b:b + GUARD] == 0xEE) and np.all(got[b + GUARD + n_bytes:b + n_bytes + 2 * GUARD] == 0xEE), \
            "wrote into the guard bytes"
        return got[b + GUARD:b + GUARD + n_bytes].copy()
    return d, p + GUARD, read


def make_spans(specs):
    spans = np.zeros(len(specs), dtype=abi.CRC_SPAN_DTYPE)
    for i, (off, ln, init) in enumerate(specs):
        spans["offset"][i], spans["n_bytes"][i], spans["init"][i] = off, ln, init
    return spans


def device_spans(be, spans, data, phase=0):
    d_d, p_d, _ = be.dev(data, phase)
    d_c, p_c, read = guarded(be, 4 * len(spans))
    be.eng.crc32_spans_device(spans, p_d, len(data), p_c)
    return read().view(np.uint32)


def want_spans(spans, data):
    raw = data.tobytes()
    return np.array([zlib.crc32(raw[int(s["offset"]):int(s["offset"]) + int(s["n_bytes"])], int(s["init"])) for s in spans],
                    dtype=np.uint32)


def assert_spans(be, spans, data, phase=0, host_form=False):
    want = want_spans(spans, data)
    got = device_spans(be, spans, data, phase)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"span {bad[0]} {spans[bad[0]]} buffer phase {phase}: {got[bad[0]]:#x} != {want[bad[0]]:#x}"
    if host_form:
        assert np.array_equal(be.eng.crc32_spans(spans, data), want)


def pack_items(rng, specs, phases=None):
    """specs: (kind, meta_len, data_len) -> (items with out_offset laid out from 0, data buffer, [(meta, data)], size)"""
    items = np.zeros(len(specs), dtype=abi.SNAP_ITEM_DTYPE)
    chunks, pos, parts = [], 0, []

    def put(ln, phase):
        nonlocal pos
        pad = int(rng.integers(0, 5)) if phase is None else (phase - pos) % 16
        chunks.append(bytes(pad)); pos += pad
        p = rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes()
        chunks.append(p); pos += ln
        return pos - ln, p
    for i, (kind, ml, dl) in enumerate(specs):
        mp, dp = (None, None) if phases is None else phases[i]
        m_off, meta = put(ml, mp)
        d_off, data = put(dl, dp)
        items["kind"][i], items["meta_len"][i], items["meta_offset"][i] = kind, ml, m_off
        items["data_offset"][i], items["data_bytes"][i] = d_off, dl
        parts.append((meta, data))
    return items, np.frombuffer(b"".join(chunks) + bytes(3), dtype=np.uint8).copy(), parts


def device_build(be, items, data, src_phase=0, dst_phase=0, with_crcs=True):
    """-> (the bytes of all images, laid out back to back, the crcs) through rgb_snapshot_build_device"""
    items, size = be.engine.snapshot_layout(items)
    d_d, p_d, _ = be.dev(data, src_phase)
    d_o, p_o, read_out = guarded(be, size, dst_phase)
    d_c, p_c, read_crcs = guarded(be, 4 * len(items))
    be.eng.snapshot_build_device(items, p_d, len(data), p_o, size, p_c if with_crcs else 0)
    return read_out().tobytes(), read_crcs().view(np.uint32)


def assert_images(be, items, data, parts, src_phase=0, dst_phase=0):
    want = b"".join(ref_image(int(it["kind"]), m, d) for it, (m, d) in zip(items, parts))
    got, crcs = device_build(be, items, data, src_phase, dst_phase)
    assert first_diff(got, want) is None, f"phases {src_phase}, {dst_phase}: {first_diff(got, want)}"
    laid, _ = be.engine.snapshot_layout(items)
    for it, crc in zip(laid, crcs):                                       # d_crcs equals the header field
        o = int(it["out_offset"])
        assert struct.unpack(">I", want[o + 5:o + 9])[0] == int(crc)
    return want


def make_files(specs):
    files = np.zeros(len(specs), dtype=abi.SNAP_FILE_DTYPE)
    for i, (off, n, kind, flags) in enumerate(specs):
        files["offset"][i], files["n_bytes"][i], files["kind"][i], files["flags"][i] = off, n, kind, flags
    return files


def pack_files(rng, blobs):
    """blobs: (bytes, kind, flags) -> (files, the files buffer) with random gaps between the files"""
    chunks, pos, specs = [], 0, []
    for blob, kind, flags in blobs:
        pad = int(rng.integers(0, 6))
        chunks.append(bytes(rng.integers(0, 256, size=pad, dtype=np.uint8))); pos += pad
        specs.append((pos, len(blob), kind, flags))
        chunks.append(blob); pos += len(blob)
    return make_files(specs), np.frombuffer(b"".join(chunks) + b"\x55" * 5, dtype=np.uint8).copy()


def device_validate(be, files, buf, phase=0):
    d_f, p_f, _ = be.dev(buf, phase)
    d_i, p_i, read = guarded(be, abi.SNAP_INFO_DTYPE.itemsize * len(files))
    be.eng.snapshot_validate_device(files, p_f, len(buf), p_i)
    return read().view(abi.SNAP_INFO_DTYPE)


def assert_rows(be, files, buf, phase=0, host_form=False):
    raw = buf.tobytes()
    want = [ref_info(raw, int(f["offset"]), int(f["n_bytes"]), int(f["kind"]), bool(f["flags"] & abi.SNAP_META_ONLY))
            for f in files]
    infos = device_validate(be, files, buf, phase)
    got = rows_as_tuples(infos)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"file {i} {files[i]}: {g} != {w}"
    assert np.all(infos["_pad"] == 0)
    if host_form:
        assert rows_as_tuples(be.eng.snapshot_validate(files, buf)) == want
    return got


# ------------------------------------------------------------------------------------------ the checks: spans

def check_spans_every_length_and_phase(be):
    rng = np.random.default_rng(500)
    buf = rng.integers(0, 256, size=16 * 8 + 16 + 600, dtype=np.uint8)
    rnd = int(rng.integers(1, 1 << 32))
    for phase in range(16):
        specs = [(phase + 16 * (ln % 8), ln, init) for ln in range(601) for init in (0, 0xFFFFFFFF, rnd)]
        assert_spans(be, make_spans(specs), buf, host_form=phase == 7)


def check_spans_boundaries(be):
    rng = np.random.default_rng(510)
    lens = [t + k for t in TIERS for k in (-1, 0, 1)] + [B - 1, B, B + 1, B + 15, B + 16, 2 * B - 1, 2 * B + 1]
    buf = rng.integers(0, 256, size=max(lens) + 32, dtype=np.uint8)
    rnd = int(rng.integers(1, 1 << 32))
    for phase in (0, 3):
        specs = [(off, ln, init) for ln in lens for off in (0, 13) for init in (0, rnd)]
        assert_spans(be, make_spans(specs), buf, phase, host_form=phase == 3)


def check_spans_second_combine_round(be):
    """257 blocks + 3 bytes: the per-item join of the blocks goes a second round of 256"""
    rng = np.random.default_rng(520)
    buf = rng.integers(0, 256, size=257 * B + 3 + 5, dtype=np.uint8)
    assert_spans(be, make_spans([(5, 257 * B + 3, 0x1234ABCD), (0, 257 * B + 3, 0), (2, 40, 7)]), buf, 0)


def check_span_batches(be):
    rng = np.random.default_rng(530)
    buf = rng.integers(0, 256, size=3 * B + 7 + 4096, dtype=np.uint8)
    assert len(device_spans(be, make_spans([]), buf)) == 0                                  # n = 0
    assert len(be.eng.crc32_spans(make_spans([]), buf)) == 0
    assert_spans(be, make_spans([(11, 1000, 5)]), buf, host_form=True)                      # n = 1
    for n in (257, 513):
        specs = [(int(rng.integers(0, 4000)), int(rng.integers(0, 2000)), int(rng.integers(0, 1 << 32))) for _ in range(n)]
        assert_spans(be, make_spans(specs), buf, n % 16)
    assert_spans(be, make_spans([(int(rng.integers(0, 5000)), 0, int(rng.integers(0, 1 << 32))) for _ in range(70)]), buf)
    for at in (0, 150, 300):                                                                # one long span among short ones
        specs = [(int(rng.integers(0, 5000)), int(rng.integers(0, 41)), int(rng.integers(0, 1 << 32))) for _ in range(300)]
        specs.insert(at, (9, 3 * B + 7, 0xDEADBEEF))
        assert_spans(be, make_spans(specs), buf, 1, host_form=at == 150)
    for ln in (100, 3 * B + 7):                                                             # the same bytes, two starting values
        assert_spans(be, make_spans([(3, ln, 0), (3, ln, 0x80000001), (3, ln, 0)]), buf)


def check_chain_law(be):
    """erlang:crc32(PartialCrc0, Chunk) chained over a buffer cut at random points = the CRC of the whole"""
    rng = np.random.default_rng(540)
    whole = rng.integers(0, 256, size=2 * B + 4321, dtype=np.uint8)
    cuts = sorted(set([0, len(whole)] + [int(x) for x in rng.integers(0, len(whole), size=9)] + [B + 7, B + 7]))
    crc = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        crc = int(device_spans(be, make_spans([(a, b - a, crc)]), whole, a % 16)[0])
    assert crc == zlib.crc32(whole.tobytes())


def check_span_refusals(be):
    buf = np.arange(200, dtype=np.uint8)
    for bad in ((190, 11, 0), (201, 0, 0), ((1 << 64) - 4, 8, 0), (0, 1 << 63, 0)):
        spans = make_spans([(0, 10, 0), bad, (5, 5, 0)])
        d_d, p_d, _ = be.dev(buf)
        d_c, p_c, read = guarded(be, 12)
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.crc32_spans_device(spans, p_d, len(buf), p_c)
        assert e.value.code == E_INVAL and np.all(read() == 0xEE), "refused, but the output was touched"
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.crc32_spans(spans, buf)
        assert e.value.code == E_INVAL


# ------------------------------------------------------------------------------------------ the checks: images

SMALL_SPECS = [(SNAPSHOT, m, d) for m in range(41) for d in range(41)] + \
              [(INDEXES, 0, d) for d in (0, 1, 15, 16, 17)]


def check_images_small(be):
    rng = np.random.default_rng(600)
    items, data, parts = pack_items(rng, SMALL_SPECS + [(INDEXES, 0, B + 1)])
    want = assert_images(be, items, data, parts)
    out, crcs = be.eng.snapshot_build(items, data)                                          # host-buffer form
    assert first_diff(out.tobytes(), want) is None
    # ... and into a caller's buffer at scattered places: only the images' own bytes are written
    laid, size = be.engine.snapshot_layout(items[:50], 7)
    laid["out_offset"][25:] += 11
    room = np.full(size + 11 + 9, 0xEE, dtype=np.uint8)
    be.eng.snapshot_build(laid, data, out=room)
    expect = np.full(len(room), 0xEE, dtype=np.uint8)
    for it, (m, d) in zip(laid, parts):
        img = ref_image(int(it["kind"]), m, d)
        expect[int(it["out_offset"]):int(it["out_offset"]) + len(img)] = np.frombuffer(img, dtype=np.uint8)
    assert np.array_equal(room, expect)


def check_images_phases(be):
    rng = np.random.default_rng(610)
    phases = [(int(rng.integers(0, 16)), int(rng.integers(0, 16))) for _ in SMALL_SPECS]
    for k in range(256):                                                                    # every pair once at least
        phases[k] = (k % 16, k // 16)
    items, data, parts = pack_items(rng, SMALL_SPECS, phases)
    laid, _ = be.engine.snapshot_layout(items)
    assert len(set(int(o) % 16 for o in laid["out_offset"])) == 16, "the batch misses an output phase"
    for sp, dp in [(p, (p * 7 + 3) % 16) for p in range(16)]:
        assert_images(be, items, data, parts, sp, dp)


def check_images_blocks(be):
    rng = np.random.default_rng(620)
    specs = [(SNAPSHOT, m, d) for d in (B - 1, B, B + 1, 3 * B - 1, 3 * B, 3 * B + 1) for m in (0, 5, 400, 2000)]
    specs += [(SNAPSHOT, 16384 + 3, 100), (SNAPSHOT, B + 9, B + 2), (INDEXES, 0, 3 * B + 1), (SNAPSHOT, 33, 16383)]
    specs += [(SNAPSHOT, t + k, t2 + k) for t in TIERS for t2 in TIERS for k in (-1, 0)]
    items, data, parts = pack_items(rng, specs)
    assert_images(be, items, data, parts, 3, 9)


def check_build_round_trip(be):
    rng = np.random.default_rng(630)
    specs = [(SNAPSHOT, 0, 0), (SNAPSHOT, 40, 0), (SNAPSHOT, 0, 40), (SNAPSHOT, 300, 5000), (INDEXES, 0, 0), (INDEXES, 0, 900),
             (SNAPSHOT, 77, 2 * B + 5), (INDEXES, 0, B + 1)]
    items, data, parts = pack_items(rng, specs)
    image, crcs = be.eng.snapshot_build(items, data)
    laid, size = be.engine.snapshot_layout(items)
    assert size == len(image)
    ends = list(laid["out_offset"][1:]) + [size]
    files = make_files([(int(it["out_offset"]), int(end) - int(it["out_offset"]), int(it["kind"]), flags)
                        for it, end in zip(laid, ends) for flags in (0, abi.SNAP_META_ONLY)])
    rows = assert_rows(be, files, image, host_form=True)
    for k, (it, (m, d)) in enumerate(zip(laid, parts)):
        for row in rows[2 * k:2 * k + 2]:
            status, version, stored, computed, m_off, m_len, d_off, d_len = row
            assert (status, version, stored) == (abi.SNAP_OK, 1, int(crcs[k]))
            head = 13 if int(it["kind"]) == SNAPSHOT else 9
            assert (m_len, d_off, d_len) == (len(m), int(it["out_offset"]) + head + len(m), len(d))
            assert image[d_off:d_off + d_len].tobytes() == d and image[m_off:m_off + m_len].tobytes() == m
        assert rows[2 * k][3] == int(crcs[k]) and rows[2 * k + 1][3] == 0


def check_build_refusals(be):
    rng = np.random.default_rng(640)
    items, data, parts = pack_items(rng, [(SNAPSHOT, 10, 20), (INDEXES, 0, 30), (SNAPSHOT, 5, 5)])
    laid, size = be.engine.snapshot_layout(items)

    def refused(its, out_bytes=size):
        d_d, p_d, _ = be.dev(data)
        d_o, p_o, read = guarded(be, size)
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.snapshot_build_device(its, p_d, len(data), p_o, out_bytes)
        assert e.value.code == E_INVAL and np.all(read() == 0xEE), "refused, but the output was touched"
        out = np.full(size, 0xEE, dtype=np.uint8)
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.snapshot_build(its, data, out=out[:out_bytes])
        assert e.value.code == E_INVAL and np.all(out == 0xEE)

    refused(laid, size - 1)                                               # the last image does not fit
    for field, i, value in (("kind", 1, 2), ("meta_len", 1, 1), ("meta_offset", 0, len(data) - 9), ("data_bytes", 2, len(data)),
                            ("data_offset", 2, (1 << 64) - 2), ("out_offset", 0, (1 << 64) - 20), ("data_bytes", 1, (1 << 64) - 5)):
        bad = laid.copy(); bad[field][i] = value
        refused(bad)


# ------------------------------------------------------------------------------------------ the checks: files

def smallest_files(rng):
    """Every status of both modes from the smallest file that produces it"""
    meta, data = rng.bytes(6), rng.bytes(20)
    snap, idx = ref_image(SNAPSHOT, meta, data), ref_image(INDEXES, b"", data)
    empty_crc0 = struct.pack(">4sBI", b"RASN", 1, 0)                      # 9 bytes, Crc 0 = crc32(<<>>): BAD_META

    def with_meta_size(total, ms):
        body = struct.pack(">I", ms) + rng.bytes(total - 13)
        return struct.pack(">4sBI", b"RASN", 1, zlib.crc32(body)) + body
    blobs = [b"", snap[:8], snap[:9], empty_crc0, b"RASI" + snap[4:], b"RASX" + snap[4:], b"XASN" + snap[4:], snap[:3],
             snap[:4] + b"\x00" + snap[5:], snap[:4] + b"\x02" + snap[5:], snap[:4] + b"\x02" + snap[5:9],
             snap[:4] + b"\xff" + snap[5:11], snap[:10], snap[:11], snap[:12], snap[:13], snap,
             struct.pack(">4sBI", b"RASN", 1, zlib.crc32(b"abc")) + b"abc",                 # CRC good, 3 bytes behind it
             with_meta_size(13, 0), with_meta_size(13, 1), with_meta_size(40, 27), with_meta_size(40, 28),
             with_meta_size(40, 0xFFFFFFFF),
             # precedence: a version fault hides a bad CRC; a bad CRC hides bad meta
             snap[:4] + b"\x03" + b"\x00\x00\x00\x01" + snap[9:],
             struct.pack(">4sBI", b"RASN", 1, 12345) + struct.pack(">I", 999) + b"xy",
             idx, idx[:9], idx[:8], struct.pack(">4sBI", b"RASI", 1, 0), idx[:4] + b"\x00" + idx[5:], idx[:-1],
             b"RASN" + idx[4:], b"\x83h\x02a\x01a\x02",                                   # a legacy indexes file: no header
             snap[:5] + b"\x00\x00\x00\x00" + snap[9:]]                                    # a stored Crc of 0 is not "unchecked"
    return [(b, kind, flags) for b in blobs for kind in (SNAPSHOT, INDEXES) for flags in (0, abi.SNAP_META_ONLY)]


def check_validate_statuses(be):
    rng = np.random.default_rng(700)
    blobs = smallest_files(rng)
    files, buf = pack_files(rng, blobs)
    for phase in (0, 7):
        rows = assert_rows(be, files, buf, phase, host_form=phase == 7)
    seen = {(int(f["kind"]), int(f["flags"]), r[0]) for f, r in zip(files, rows)}
    for kind in (SNAPSHOT, INDEXES):
        for flags, statuses in ((0, (0, 1, 2, 3)), (abi.SNAP_META_ONLY, (0, 1, 2, 5))):
            for st in statuses + ((abi.SNAP_BAD_META,) if kind == SNAPSHOT else ()):
                assert (kind, flags, st) in seen, f"no file gives status {st} (kind {kind}, flags {flags})"
    by_blob = {(blobs[i][0], blobs[i][1], blobs[i][2]): rows[i][0] for i in range(len(blobs))}
    assert by_blob[(struct.pack(">4sBI", b"RASN", 1, 0), SNAPSHOT, 0)] == abi.SNAP_BAD_META
    assert by_blob[(blobs[-4][0], SNAPSHOT, 0)] == abi.SNAP_CHECKSUM


def check_validate_flipped_bits(be):
    rng = np.random.default_rng(710)
    meta, data = rng.bytes(50), rng.bytes(3 * B + 77 - 4 - 50)            # 3 blocks + 77 bytes behind byte 9
    good = ref_image(SNAPSHOT, meta, data)
    n = len(good)
    at = [9, n - 1] + [n - k * B - 1 for k in (1, 2, 3)] + [n - k * B for k in (1, 2, 3)]
    blobs = [(good, SNAPSHOT, 0)]
    for pos in at:
        bad = bytearray(good); bad[pos] ^= 1 << int(rng.integers(0, 8))
        blobs.append((bytes(bad), SNAPSHOT, 0))
    small = ref_image(SNAPSHOT, rng.bytes(9), rng.bytes(700))
    for pos in (9, len(small) - 1, 400):
        bad = bytearray(small); bad[pos] ^= 0x40
        blobs.append((bytes(bad), SNAPSHOT, 0))
    files, buf = pack_files(rng, blobs)
    rows = assert_rows(be, files, buf, 5)
    assert [r[0] for r in rows] == [abi.SNAP_OK] + [abi.SNAP_CHECKSUM] * (len(blobs) - 1)


def check_validate_independent(be):
    """300 files, every fifth one bad: the good rows are those of the all-good batch"""
    rng = np.random.default_rng(720)
    good = []
    for k in range(300):
        kind = INDEXES if k % 7 == 3 else SNAPSHOT
        meta = rng.bytes(int(rng.integers(0, 60))) if kind == SNAPSHOT else b""
        size = (B + 100 if k == 40 else 17000 if k == 41 else int(rng.integers(0, 1500)))
        good.append((ref_image(kind, meta, rng.bytes(size)), kind, abi.SNAP_META_ONLY if k % 11 == 0 else 0))
    mixed = list(good)
    for k in range(0, 300, 5):
        blob, kind, flags = good[k]
        how = (k // 5) % 4
        bad = bytearray(blob)
        if how == 0:
            bad[len(bad) - 1 if len(bad) > 9 else 5] ^= 0x20
        elif how == 1:
            bad[4] = 7
        elif how == 2:
            bad[1] = ord("B")
        else:
            bad = bad[:int(rng.integers(0, 9))]
        mixed[k] = (bytes(bad), kind, flags)
    chunks_good, chunks_mixed, specs_good, specs_mixed, pos = [], [], [], [], 0
    for (g, kind, flags), (m, _, _) in zip(good, mixed):                  # the same offsets in both buffers
        specs_good.append((pos, len(g), kind, flags)); specs_mixed.append((pos, len(m), kind, flags))
        chunks_good.append(g); chunks_mixed.append(m + bytes(len(g) - len(m)))
        pos += len(g)
    rows_good = assert_rows(be, make_files(specs_good), np.frombuffer(b"".join(chunks_good), dtype=np.uint8).copy())
    rows_mixed = assert_rows(be, make_files(specs_mixed), np.frombuffer(b"".join(chunks_mixed), dtype=np.uint8).copy())
    assert all(r[0] == abi.SNAP_OK for r in rows_good)
    for k in range(300):
        if k % 5:
            assert rows_mixed[k] == rows_good[k], k
        elif not (good[k][2] and (k // 5) % 4 == 0):                      # (META_ONLY does not see a flipped payload bit)
            assert rows_mixed[k][0] != abi.SNAP_OK, k


def check_validate_refusals(be):
    buf = np.frombuffer(ref_image(SNAPSHOT, b"meta", b"data" * 10), dtype=np.uint8).copy()
    assert len(device_validate(be, make_files([]), buf)) == 0             # n = 0
    for bad in ((0, len(buf) + 1, SNAPSHOT, 0), (len(buf) + 1, 0, SNAPSHOT, 0), (0, 10, 2, 0), (0, 10, INDEXES, 2),
                ((1 << 64) - 1, 2, SNAPSHOT, 0)):
        files = make_files([(0, len(buf), SNAPSHOT, 0), bad])
        d_f, p_f, _ = be.dev(buf)
        d_i, p_i, read = guarded(be, 96)
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.snapshot_validate_device(files, p_f, len(buf), p_i)
        assert e.value.code == E_INVAL and np.all(read() == 0xEE), "refused, but the output was touched"
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.snapshot_validate(files, buf)
        assert e.value.code == E_INVAL


CHECKS = [check_spans_every_length_and_phase, check_spans_boundaries, check_spans_second_combine_round, check_span_batches,
          check_chain_law, check_span_refusals, check_images_small, check_images_phases, check_images_blocks,
          check_build_round_trip, check_build_refusals, check_validate_statuses, check_validate_flipped_bits,
          check_validate_independent, check_validate_refusals]


# ------------------------------------------------------------------------------------------ CPU (emulation)

@pytest.mark.parametrize("check", CHECKS, ids=[c.__name__[6:] for c in CHECKS])
def test_emu(emu, check):
    check(emu)


SCHEDULE_CHECKS = [check_span_batches, check_images_blocks, check_validate_independent, check_spans_second_combine_round]


@pytest.mark.parametrize("sched", PERMUTED_SCHEDULES)
def test_emu_under_permuted_schedules(emu, sched):
    """Every pass of the snapshot kernels is its own launch "so that no workgroup ever waits for another", and on the
    emulation's own order (workgroups 0, 1, 2, ..., lanes 0 .. 255) a workgroup that read what a lower-numbered one
    wrote in the same launch would still be right.  The checks that span many workgroups -- batches of 257 and 513
    items, pieces of several blocks, 300 files, the second join round -- with workgroups and lanes reversed and permuted
    (tests/emu_schedule.py); the referee stays zlib."""
    with schedule(emu.engine, sched):
        for check in SCHEDULE_CHECKS:
            try:
                check(emu)
            except AssertionError as e:
                raise AssertionError(f"{check.__name__}: {e}") from e


def test_abi_mirror():
    hdr = open(os.path.join(ROOT, "include", "ra_gpu_wal.h")).read()
    flat = " ".join(hdr.split())
    for name, val in (("RGB_SNAP_KIND_SNAPSHOT", SNAPSHOT), ("RGB_SNAP_KIND_INDEXES", INDEXES),
                      ("RGB_SNAP_HEADER_BYTES", abi.SNAP_HEADER_BYTES), ("RGB_SNAP_META_HEADER_BYTES", abi.SNAP_META_HEADER_BYTES),
                      ("RGB_SNAP_META_ONLY", abi.SNAP_META_ONLY), ("RGB_SNAP_OK", abi.SNAP_OK),
                      ("RGB_SNAP_INVALID_FORMAT", abi.SNAP_INVALID_FORMAT), ("RGB_SNAP_INVALID_VERSION", abi.SNAP_INVALID_VERSION),
                      ("RGB_SNAP_CHECKSUM", abi.SNAP_CHECKSUM), ("RGB_SNAP_BAD_META", abi.SNAP_BAD_META),
                      ("RGB_SNAP_EOF", abi.SNAP_EOF)):
        assert int(flat.split(f"#define {name} ")[1].split()[0].rstrip("u")) == val, name
    src = open(os.path.join(ROOT, "ra_amd", "csrc", "rgb_segment.hip")).read()
    assert f"SNAP_T8 = {TIERS[0] - 1}u" in src and f"SNAP_T16 = {TIERS[1]}u" in src and f"SNAP_TBLOCK = {TIERS[2]}u" in src
    assert "SNAP_BLOCK = STREAM_BLOCK" in src
    assert abi.SNAP_INFO_DTYPE.fields["data_offset"][1] == 32 and abi.SNAP_ITEM_DTYPE.fields["out_offset"][1] == 32


def test_gf2_referee_on_short_buffers():
    """The arithmetic the 2^32 test takes its expected value from, against zlib on buffers of a few KiB:
    raw(A ++ B) = raw(A) x^(8 |B|) ^ raw(B), leading zeros neutral, crc(M, init) = ~(~init x^(8 |M|) ^ raw(M))"""
    rng = np.random.default_rng(800)
    for la, lz, lb in ((3, 4000, 5), (100, 0, 3000), (1, 8191, 1), (0, 5000, 2)):
        a, b = rng.bytes(la), rng.bytes(lb)
        assert sparse_crc([(0, a), (la + lz, b)], la + lz + lb, 0x1234) == zlib.crc32(a + bytes(lz) + b, 0x1234)
    assert raw_crc(bytes(777) + b"xyz") == raw_crc(b"xyz")


def sparse_crc(pieces, total, init):
    """crc32 of a zero-filled buffer of `total` bytes holding `pieces` = [(offset, bytes)], by the combine arithmetic"""
    raw = 0
    for off, b in pieces:
        raw ^= gf2_mulmod(raw_crc(b), gf2_xpow8(total - off - len(b)))
    return ~(gf2_mulmod(~init & 0xFFFFFFFF, gf2_xpow8(total)) ^ raw) & 0xFFFFFFFF


def test_snapshot_kernels_resources():
    """hipcc's resource remarks for gfx950 (no GPU needed), through tests/test_kernel_resources.py: the rgb_snap_ kernels
    are the eleven the unit declares -- group x {8, 16, 64 lanes} x {read, copy}, block x {read, copy}, finish x {spans,
    build, validate} -- each without scratch or spills, 20 KiB of LDS, at least 7 wavefronts per SIMD; and the other
    gates' counts still hold."""
    from test_kernel_resources import segment_usage
    usage = segment_usage()
    names = sorted(k for k in usage if "rgb_snap_" in k)
    assert len(names) == 11, names
    assert sum("rgb_snap_group_kernel" in k for k in names) == 6 and sum("rgb_snap_block_kernel" in k for k in names) == 2
    assert sum("rgb_snap_finish_kernel" in k for k in names) == 3
    for k in names:
        u = usage[k]
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, f"{k}: {u}"
        assert u["Occupancy"] >= 7 and u["LDS Size"] <= 20 * 1024 + 64, f"{k}: {u}"
    for sub, count in (("rgb_seg_", 8), ("rgb_compact_", 9), ("rgb_read_", 9), ("rgb_flush_", 7)):
        assert sum(sub in k for k in usage) == count, sub
    assert not any("rgb_prep_" in k for k in usage)


def test_snapshot_descriptors_under_sanitizers(tmp_path):
    """The descriptor validation of the three calls and rgb_snapshot_layout -- host-only code of rgb_segment_host.cpp --
    compiled with AddressSanitizer + UBSan into a stand-alone program and run over malformed descriptor arrays, each in
    an exactly-sized heap block; the answers are compared with the same rules written here."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "snapshot_harness"
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-o", str(exe),
           os.path.join(ROOT, "tests", "native", "snapshot_harness.cpp"),
           os.path.join(ROOT, "ra_amd", "csrc", "rgb_segment_host.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert built.returncode == 0, built.stderr
    M = 1 << 64
    rng = np.random.default_rng(810)

    def inside(off, n, room):
        return off <= room and n <= room - off

    def value(limit):
        r = rng.random()
        if r < 0.7:
            return int(rng.integers(0, limit))
        return [limit, limit + 1, M - 1, M - int(rng.integers(1, 40)), 1 << 63, 0][int(rng.integers(0, 6))]

    paths, want = [], []
    for trial in range(400):
        mode, n = trial % 3, int(rng.integers(0, 6)) if trial % 10 else 0
        room, out_room, base = int(rng.integers(0, 4000)), int(rng.integers(0, 6000)), value(3000)
        rc, total = 0, 0
        if mode == 0:
            desc = np.zeros(n, dtype=abi.CRC_SPAN_DTYPE)
            for i in range(n):
                desc["offset"][i], desc["n_bytes"][i], desc["init"][i] = value(room // 2 + 1), value(room // 2 + 1), 5
                if rc == 0:
                    rc = 0 if inside(int(desc["offset"][i]), int(desc["n_bytes"][i]), room) else E_INVAL
                total += int(desc["n_bytes"][i])
            line = (rc, 0 if rc else min(total, M - 1))
        elif mode == 1:
            desc = np.zeros(n, dtype=abi.SNAP_ITEM_DTYPE)
            pos, mix = base, 0
            for i in range(n):
                kind = int(rng.integers(0, 2)) if rng.random() < 0.9 else 2
                ml = 0 if kind == 1 and rng.random() < 0.8 else int(rng.integers(0, 50))
                desc["kind"][i], desc["meta_len"][i] = kind, ml
                desc["meta_offset"][i], desc["data_offset"][i] = value(room // 2 + 1), value(room // 2 + 1)
                desc["data_bytes"][i], desc["out_offset"][i] = value(room // 2 + 1), value(out_room // 2 + 1)
                size = (13 if kind == 0 else 9) + ml + int(desc["data_bytes"][i])
                ok = size < M
                if rc == 0 and not (kind in (0, 1) and not (kind == 1 and ml) and
                                    inside(int(desc["meta_offset"][i]), ml, room) and
                                    inside(int(desc["data_offset"][i]), int(desc["data_bytes"][i]), room) and ok and
                                    inside(int(desc["out_offset"][i]), size, out_room)):
                    rc = E_INVAL
                total += size
                mix = (mix * 31 + pos) % M                                # the layout: back to back from base
                pos = (pos + (size if ok else 0)) % M
            line = (rc, 0 if rc else min(total, M - 1), pos, mix)
        else:
            desc = np.zeros(n, dtype=abi.SNAP_FILE_DTYPE)
            for i in range(n):
                desc["offset"][i], desc["n_bytes"][i] = value(room // 2 + 1), value(room // 2 + 1)
                desc["kind"][i] = int(rng.integers(0, 2)) if rng.random() < 0.9 else 7
                desc["flags"][i] = int(rng.integers(0, 2)) if rng.random() < 0.9 else 2
                if rc == 0 and not (int(desc["kind"][i]) in (0, 1) and int(desc["flags"][i]) in (0, 1) and
                                    inside(int(desc["offset"][i]), int(desc["n_bytes"][i]), room)):
                    rc = E_INVAL
                if not desc["flags"][i] & 1:
                    total += int(desc["n_bytes"][i])
            line = (rc, 0 if rc else min(total, M - 1))
        path = tmp_path / f"d{trial}.bin"
        path.write_bytes(struct.pack("<IIQQQ", mode, n, room, out_room, base) + desc.tobytes())
        paths.append(str(path)); want.append(line)
    run = subprocess.run([str(exe)] + paths, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in run.stdout.splitlines()]
    assert got == want
    assert sum(1 for w in want if w[0] == 0) > 60 and sum(1 for w in want if w[0]) > 60


# ------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=[c.__name__[6:] for c in CHECKS])
def test_gpu(gpu, check):
    check(gpu)


@pytest.mark.gpu
def test_gpu_span_beyond_32_bits(gpu):
    """One span of 2^32 + 65 537 + 5 bytes in a zero-filled device buffer with a few random bytes near its start, at a
    block boundary and at its end; the expected value is the combine arithmetic pinned by
    test_gf2_referee_on_short_buffers."""
    import torch
    n = (1 << 32) + 65537 + 5
    rng = np.random.default_rng(820)
    t = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    base = 3                                                              # the span's own alignment
    pieces = [(1, rng.bytes(9)), (n - 40 * B - 4, rng.bytes(8)), (n - B - 3, rng.bytes(7)), (n - 5, rng.bytes(5))]
    for off, b in pieces:
        t[base + off:base + off + len(b)] = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy())
    d_c = torch.full((4,), 0x6E6E6E6E, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    init = 0x89ABCDEF
    spans = make_spans([(base, n, init), (base, 100, 0)])
    gpu.eng.crc32_spans_device(spans, t.data_ptr(), n + 16, d_c.data_ptr())
    gpu.eng.synchronize()
    got = d_c.cpu().numpy().view(np.uint32)
    assert int(got[0]) == sparse_crc(pieces, n, init), hex(int(got[0]))
    assert int(got[1]) == zlib.crc32(bytes(1) + pieces[0][1] + bytes(90))
    assert int(got[2]) == 0x6E6E6E6E and int(got[3]) == 0x6E6E6E6E
