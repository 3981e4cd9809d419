"""Batched CRC-32 for segment files and snapshot checksums (include/ra_gpu_wal.h, "segments and snapshots";
ra_amd/csrc/rgb_segment.hip, rgb_segment_host.cpp).

Referee: Python's zlib.crc32 -- the function erlang:crc32 is -- and struct.pack over the file format as the
reference source states it:
  src/ra_log_segment.erl:41-45    "RASG", version 2, 8 header bytes, index records of 32 bytes (v2) / 28 bytes (v1)
  src/ra_log_segment.erl:1118-1122 Header = <<"RASG", Version:16, MaxCount:16>>
  src/ra_log_segment.erl:1211-1219 <<Idx:64, Term:64, DataOffset:64 (v1: 32), Length:32, Crc:32>>, big-endian
  src/ra_log_segment.erl:228, 247  IndexSize = MaxCount * record size, data_start = 8 + IndexSize
  src/ra_log_segment.erl:1240-1248 compute_checksum (0 when switched off), validate_checksum (0 = not checked)
  src/ra_log_snapshot.erl:57, 107  erlang:crc32(Data), erlang:crc32(PartialCrc0, Chunk)
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
from ra_amd import abi, engine as product_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL = -1
STREAM_BLOCK = 65536           # rgb_segment.hip: bytes of a long buffer per workgroup step
ROUND = 4096                   # ... and per round of its 256 lanes


# ------------------------------------------------------------------------------------------ referee

def python_segment(entries, payloads, max_count, checksums=True, version=2) -> bytes:
    """The file image by struct.pack + zlib (see the module docstring for the source lines)."""
    rec = 32 if version == 2 else 28
    pos = 8 + max_count * rec
    index = []
    for (idx, term), p in zip(entries, payloads):
        crc = zlib.crc32(p) if checksums else 0
        index.append(struct.pack(">QQQII" if version == 2 else ">QQIII", idx, term, pos, len(p), crc))
        pos += len(p)
    return struct.pack(">4sHH", b"RASG", version, max_count) + b"".join(index) + \
        bytes(rec * (max_count - len(payloads))) + b"".join(payloads)


def pack_entries(rng, lens, phases=None, tail=0):
    """Payloads of `lens` in one data buffer, each at a chosen address phase mod 16 (random gaps otherwise)."""
    entries = np.zeros(len(lens), dtype=abi.SEG_ENTRY_DTYPE)
    chunks, pos, payloads = [], 0, []
    for i, ln in enumerate(lens):
        pad = int(rng.integers(0, 7)) if phases is None else (phases[i] - pos) % 16
        chunks.append(bytes(pad)); pos += pad
        p = rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes()
        payloads.append(p)
        entries["index"][i], entries["term"][i] = 1000 + i, 1 + i % 5
        entries["data_offset"][i], entries["data_len"][i] = pos, ln
        chunks.append(p); pos += ln
    data = np.frombuffer(b"".join(chunks) + bytes(tail), dtype=np.uint8).copy()
    return entries, data, payloads


def force_group(entries, data, small):
    """Pad the data buffer so that its mean per entry selects the lane-group width: a wavefront (0), sixteen
    lanes (1) or eight (2) per entry -- the rule of rgb_crc32_device / rgb_segment_build_device."""
    n = max(1, len(entries))
    want = (2000, 600, 100)[small] * n
    if small == 2:
        assert len(data) // n <= 320, "too large for eight lanes"
        return data
    if len(data) < want:
        data = np.concatenate([data, np.zeros(want - len(data), dtype=np.uint8)])
    mean = len(data) // n
    assert (mean < 1024) == bool(small) and (small == 0 or mean > 320)
    return data


# ------------------------------------------------------------------------------------------ back ends

class Emu:
    """"Device" buffers of the emulated library are host buffers."""
    gpu = False

    def __init__(self, eng_mod):
        self.engine, self.eng = eng_mod, eng_mod.RaGpuBatch(1, 1)

    def dev(self, arr, phase=0):
        buf = np.zeros(len(arr) + 32, dtype=np.uint8)
        base = (-buf.ctypes.data) % 16 + phase
        buf[base:base + len(arr)] = arr
        return buf, buf.ctypes.data + base, base

    def get(self, buf):
        return buf

    def sync(self):
        pass

    def close(self):
        self.eng.close()


class Gpu(Emu):
    gpu = True

    def dev(self, arr, phase=0):
        import torch
        t = torch.zeros(len(arr) + 32, dtype=torch.uint8, device="cuda")
        base = (-t.data_ptr()) % 16 + phase
        t[base:base + len(arr)] = torch.from_numpy(np.ascontiguousarray(arr))
        torch.cuda.synchronize()               # the library launches on its own stream
        return t, t.data_ptr() + base, base

    def get(self, buf):
        self.eng.synchronize()
        return buf.cpu().numpy()

    def sync(self):
        self.eng.synchronize()


@pytest.fixture(scope="module")
def emu(emulated_engine):
    b = Emu(emulated_engine)
    yield b
    b.close()


@pytest.fixture(scope="module")
def gpu():
    if not os.path.exists(product_engine.LIB_PATH):
        product_engine.build()
    b = Gpu(product_engine)
    yield b
    b.close()


def device_crcs(be, entries, data, phase=0):
    d_e, p_e, _ = be.dev(entries.view(np.uint8))
    d_d, p_d, _ = be.dev(data, phase)
    d_c, p_c, b_c = be.dev(np.full(4 * len(entries), 0xEE, dtype=np.uint8))
    be.eng.crc32_device(p_e, len(entries), p_d, len(data), p_c)
    return be.get(d_c)[b_c:b_c + 4 * len(entries)].copy().view(np.uint32)


def device_stream(be, data, init, phase=0):
    d_d, p_d, _ = be.dev(data, phase)
    d_c, p_c, b_c = be.dev(np.zeros(4, dtype=np.uint8))
    be.eng.crc32_stream_device(p_d, len(data), init, p_c)
    return int(be.get(d_c)[b_c:b_c + 4].copy().view(np.uint32)[0])


def device_build(be, entries, data, max_count, flags=0, src_phase=0, dst_phase=0, slack=48):
    """-> (file bytes, bytes behind the file) through rgb_segment_build_device; the output is poisoned first."""
    offs, size = be.engine.segment_layout(entries, max_count)
    d_e, p_e, _ = be.dev(entries.view(np.uint8))
    d_f, p_f, _ = be.dev(offs.view(np.uint8))
    d_d, p_d, _ = be.dev(data, src_phase)
    d_o, p_o, b_o = be.dev(np.full(size + slack, 0xEE, dtype=np.uint8), dst_phase)
    be.eng.segment_build_device(p_e, len(entries), max_count, p_f, p_d, len(data), p_o, size + slack, flags)
    got = be.get(d_o)
    assert np.all(got[:b_o] == 0) and np.all(got[b_o + size + slack:] == 0), "wrote outside the output buffer"
    return got[b_o:b_o + size].tobytes(), got[b_o + size:b_o + size + slack]


def first_diff(a: bytes, b: bytes):
    if a == b:
        return None
    x, y = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
    if len(x) != len(y):
        return f"lengths {len(x)} != {len(y)}"
    return f"first differing byte {int(np.flatnonzero(x != y)[0])} of {len(x)}"


# ------------------------------------------------------------------------------------------ the checks

def check_known_answers(be):
    for data, want in ((b"", 0), (b"123456789", 0xCBF43926), (bytes(1 << 20), None), (b"\xff" * (1 << 20), None)):
        want = zlib.crc32(data) if want is None else want
        assert zlib.crc32(data) == want
        arr = np.frombuffer(data, dtype=np.uint8)
        assert be.eng.crc32_stream(arr, 0) == want                       # stream, host-buffer form
        assert device_stream(be, arr, 0) == want                         # stream, device form
        e = np.zeros(1, dtype=abi.SEG_ENTRY_DTYPE)
        e["data_len"] = len(data)
        assert int(be.eng.crc32(e, arr)[0]) == want                      # per entry, host-buffer form
        assert int(device_crcs(be, e, arr)[0]) == want                   # per entry, device form


def check_every_length_and_phase(be, small):
    rng = np.random.default_rng(300 + small)
    specs = [(ln, ph) for ln in range(81) for ph in range(16)]
    entries, data, payloads = pack_entries(rng, [s[0] for s in specs], [s[1] for s in specs])
    data = force_group(entries, data, small)
    want = np.array([zlib.crc32(p) for p in payloads], dtype=np.uint32)
    got = device_crcs(be, entries, data)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"len {specs[bad[0]][0]} phase {specs[bad[0]][1]}: {got[bad[0]]:#x} != {want[bad[0]]:#x}"
    assert np.array_equal(be.eng.crc32(entries, data), want)


def check_random_lengths(be, small):
    rng = np.random.default_rng(310 + small)
    if small == 2:
        lens = [0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 257] + [int(x) for x in rng.integers(0, 600, size=300)]
    elif small == 1:
        lens = [0, 1, 16, 255, 256, 257, 271, 511, 512, 513, 1023] + [int(x) for x in rng.integers(300, 1000, size=150)]
    else:
        big = [1 << 20, (1 << 20) - 1, 70001] if not be.gpu else [1 << 20, (1 << 20) - 1, (1 << 20) - 17, 70001, 999983]
        lens = [0, 1, 15, 16, 17, 1007, 1023, 1024, 1025, 1040, 4095, 4096, 4097, 65535, 65536] + big + \
               [int(x) for x in rng.integers(0, 20000 if not be.gpu else 1 << 20, size=30 if not be.gpu else 120)]
    entries, data, payloads = pack_entries(rng, lens)
    data = force_group(entries, data, small)
    want = np.array([zlib.crc32(p) for p in payloads], dtype=np.uint32)
    for phase in (0, 5):                                                  # the data buffer's own alignment
        got = device_crcs(be, entries, data, phase)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, f"entry {bad[0]} len {lens[bad[0]]} buffer phase {phase}"


STREAM_LENS = [0, 1, 15, 16, 17, 31, 32, 33, ROUND - 1, ROUND, ROUND + 1, ROUND + 15, ROUND + 16, ROUND + 17,
               STREAM_BLOCK - 1, STREAM_BLOCK, STREAM_BLOCK + 1, STREAM_BLOCK + 15, STREAM_BLOCK + 16,
               2 * STREAM_BLOCK - 1, 2 * STREAM_BLOCK + 7, 7 * STREAM_BLOCK, 13 * STREAM_BLOCK + 4099]


def check_stream(be):
    rng = np.random.default_rng(320)
    lens = STREAM_LENS + ([257 * STREAM_BLOCK + 3, 513 * STREAM_BLOCK] if be.gpu else [])   # > 256 partial values
    buf = rng.integers(0, 256, size=max(lens) + 16, dtype=np.uint8)
    rnd = int(rng.integers(1, 1 << 32))
    for ln in lens:
        for init in (0, rnd):
            for phase in (0, 3):
                data = buf[phase:phase + ln]
                want = zlib.crc32(data.tobytes(), init)
                got = device_stream(be, data, init, phase)
                assert got == want, f"len {ln} init {init:#x} phase {phase}: {got:#x} != {want:#x}"
        assert be.eng.crc32_stream(buf[:ln], rnd) == zlib.crc32(buf[:ln].tobytes(), rnd)
    # chained, split at unaligned points: crc(crc(0, A), B) == crc(A ++ B)
    whole = buf[:3 * STREAM_BLOCK + 1234]
    for cut in (1, 7, 4099, STREAM_BLOCK + 5, 2 * STREAM_BLOCK - 3, len(whole) - 9):
        a = device_stream(be, whole[:cut], 0)
        assert device_stream(be, whole[cut:], a, cut % 16) == zlib.crc32(whole.tobytes()), f"cut at {cut}"


def check_build_cases(be, small):
    rng = np.random.default_rng(330 + small)
    base = ([0, 0, 1, 2, 15, 16, 17, 40, 100, 255, 256, 257] + [int(x) for x in rng.integers(0, 320, size=60)],
            [0, 400, 511, 512, 513, 767, 1000] + [int(x) for x in rng.integers(330, 1000, size=40)],
            [0, 1007, 1024, 1025, 4096, 9000, 33000, 65537] + [int(x) for x in rng.integers(1000, 9000, size=30)])[2 - small]
    for lens, max_count, flags in (([], 16, 0), (base[:1], 1, 0), (base[3:4], 4096, 0), (base, len(base), 0),
                                   (base, 4096, 0), (base, len(base) + 3, abi.SEG_NO_CHECKSUMS), ([0, 0, 0], 7, 0)):
        entries, data, payloads = pack_entries(rng, lens)
        if lens and sum(lens):
            data = force_group(entries, data, small) if len(lens) > 4 else data
        want = python_segment([(int(e["index"]), int(e["term"])) for e in entries], payloads, max_count, not flags)
        for sp, dp in ((0, 0), (3, 9)):
            got, behind = device_build(be, entries, data, max_count, flags, sp, dp)
            assert first_diff(got, want) is None, f"n {len(lens)} max_count {max_count}: {first_diff(got, want)}"
            assert np.all(behind == 0xEE), "bytes behind the file were written"
        n = len(lens)
        assert want[8 + 32 * n:8 + 32 * max_count] == bytes(32 * (max_count - n))      # the unused index records
        out = np.full(len(want) + 40, 0xEE, dtype=np.uint8)                            # host-buffer form
        be.eng.segment_build(entries, data, max_count, flags, out=out)
        assert first_diff(out[:len(want)].tobytes(), want) is None and np.all(out[len(want):] == 0xEE)


def check_build_every_phase(be, small):
    """Every payload length of the sweep at every source phase, the whole image at several destination phases:
    consecutive payloads of odd lengths put the copies at every destination phase as well."""
    from test_wal_framing import SWEEP_LARGE, SWEEP_MID, SWEEP_SMALL
    rng = np.random.default_rng(340 + small)
    lens = (SWEEP_LARGE, SWEEP_MID, SWEEP_SMALL)[small]
    specs = [(ln + k, sp) for ln in lens for sp in range(16) for k in ((0, 1) if small else (0,))]
    entries, data, payloads = pack_entries(rng, [s[0] for s in specs], [s[1] for s in specs])
    data = force_group(entries, data, small)
    offs, _ = be.engine.segment_layout(entries, len(specs))
    assert len(set(int(o) % 16 for o in offs)) == 16, "the sweep misses a destination phase"
    want = python_segment([(int(e["index"]), int(e["term"])) for e in entries], payloads, len(specs))
    for dp in ((0, 1, 7, 8, 15) if not be.gpu else range(16)):
        got, behind = device_build(be, entries, data, len(specs), 0, (dp * 5) % 16, dp)
        assert first_diff(got, want) is None, f"destination phase {dp}: {first_diff(got, want)}"
        assert np.all(behind == 0xEE)


def check_refusals(be):
    rng = np.random.default_rng(350)
    entries, data, payloads = pack_entries(rng, [10, 200, 3000])
    size = be.engine.segment_layout(entries, 8)[1]

    def refused(ents, dat, max_count, out_len, flags=0):
        out = np.full(out_len, 0xEE, dtype=np.uint8)
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.segment_build(ents, dat, max_count, flags, out=out)
        assert e.value.code == E_INVAL and np.all(out == 0xEE), "refused, but the output was touched"

    refused(entries, data, 2, size)                        # n > max_count
    refused(entries, data, 65536, 8 + 32 * 65536 + 4000)   # max_count > 65535
    refused(entries, data, 8, size - 1)                    # output too small
    bad = entries.copy(); bad["data_len"][2] = len(data)   # payload runs past the data buffer
    refused(bad, data, 8, size + 70000)
    bad = entries.copy(); bad["data_offset"][0] = (1 << 64) - 4
    refused(bad, data, 8, size)
    refused(entries, data, 8, size, flags=2)               # unknown flag
    with pytest.raises(be.engine.RgbError) as e:
        be.eng.crc32(bad, data)
    assert e.value.code == E_INVAL
    # the device form checks what it can see without reading the entries
    d_o, p_o, b_o = be.dev(np.full(size, 0xEE, dtype=np.uint8))
    for n, mc, ob in ((3, 2, size), (3, 65536, size), (3, 8, 8 + 32 * 8 - 1)):
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.segment_build_device(p_o, n, mc, p_o, p_o, 16, p_o, ob)
        assert e.value.code == E_INVAL
    assert np.all(be.get(d_o)[b_o:b_o + size] == 0xEE), "refused, but the output was touched"
    # an entry that points outside is skipped by the kernel: nothing outside the image is written
    out_entries = entries.copy(); out_entries["data_offset"][1] = len(data) - 5
    got, behind = device_build(be, out_entries, data, 8)
    assert np.all(behind == 0xEE)


def check_round_trip(be):
    rng = np.random.default_rng(360)
    lens = [0, 5, 16, 17, 300, 1000, 4096, 7001] + [int(x) for x in rng.integers(1, 3000, size=24)]
    entries, data, payloads = pack_entries(rng, lens)
    image = be.eng.segment_build(entries, data, 64)
    recs, version, max_count, end = be.engine.segment_scan(image)
    assert (version, max_count, end, len(recs)) == (2, 64, abi.SEG_END_ZEROS, len(lens))
    offs, size = be.engine.segment_layout(entries, 64)
    assert size == len(image) and np.array_equal(recs["data_offset"], offs)
    assert np.array_equal(recs["index"], entries["index"]) and np.array_equal(recs["data_len"], entries["data_len"])
    assert [int(c) for c in recs["crc"]] == [zlib.crc32(p) for p in payloads]
    assert be.eng.segment_validate(image, recs) == len(lens)
    k = 11
    assert lens[k] > 0
    bad = image.copy(); bad[int(recs["data_offset"][k]) + lens[k] // 2] ^= 0x10
    assert be.eng.segment_validate(bad, recs) == k
    # a stored CRC of 0 is "not checked": the damaged record passes (src/ra_log_segment.erl:1245-1246)
    bad[8 + 32 * k + 28:8 + 32 * k + 32] = 0
    recs0 = be.engine.segment_scan(bad)[0]
    assert int(recs0["crc"][k]) == 0 and be.eng.segment_validate(bad, recs0) == len(lens)
    # full index: the walk ends after MaxCount records
    full = be.eng.segment_build(entries, data, len(lens))
    assert be.engine.segment_scan(full)[1:] == (2, len(lens), abi.SEG_END_FULL)
    # a hand-packed version-1 image scans to the same records (28-byte records, 32-bit DataOffset)
    v1 = python_segment([(int(e["index"]), int(e["term"])) for e in entries], payloads, 64, version=1)
    recs1, version, max_count, end = be.engine.segment_scan(v1)
    assert (version, max_count, end) == (1, 64, abi.SEG_END_ZEROS)
    for f in ("index", "term", "data_len", "crc"):
        assert np.array_equal(recs1[f], recs[f]), f
    assert np.array_equal(recs1["data_offset"], recs["data_offset"] - 64 * 4)
    assert be.eng.segment_validate(np.frombuffer(v1, dtype=np.uint8), recs1) == len(lens)
    # truncated files: the first record whose payload is cut ends the walk and is not reported as a record
    cut = int(recs["data_offset"][20]) + lens[20] - 1
    part, _, _, end = be.engine.segment_scan(image[:cut])
    assert len(part) == 20 and end == abi.SEG_END_TRUNCATED
    assert be.eng.segment_validate(image[:cut], part) == 20
    part, _, _, end = be.engine.segment_scan(image[:8 + 32 * 3 + 5])          # inside the index region
    assert len(part) == 0 and end == abi.SEG_END_TRUNCATED                   # (its payloads lie behind the cut)
    for broken in (b"RASX" + image[4:].tobytes(), image[:7].tobytes(), b"RASG\x00\x03" + image[6:].tobytes(),
                   b"RASG\x00\x00" + image[6:].tobytes()):
        with pytest.raises(be.engine.RgbError) as e:
            be.engine.segment_scan(broken)
        assert e.value.code == E_INVAL


# ------------------------------------------------------------------------------------------ CPU (emulation)

def test_abi_mirror():
    assert abi.SEG_ENTRY_DTYPE.itemsize == 32 and abi.SEG_ENTRY_DTYPE.fields["crc"][1] == 28
    assert abi.SEG_NO_CHECKSUMS == 1
    hdr = open(os.path.join(ROOT, "include", "ra_gpu_wal.h")).read()
    for name, val in (("RGB_SEG_NO_CHECKSUMS", abi.SEG_NO_CHECKSUMS), ("RGB_SEG_RECORD_BYTES", abi.SEG_RECORD_BYTES),
                      ("RGB_SEG_RECORD_BYTES_V1", abi.SEG_RECORD_BYTES_V1), ("RGB_SEG_END_TRUNCATED", abi.SEG_END_TRUNCATED),
                      ("RGB_SEG_END_CAP", abi.SEG_END_CAP), ("RGB_SEG_END_FULL", abi.SEG_END_FULL)):
        assert f"#define {name} " in hdr.replace("  ", " ").replace("  ", " ") and \
            int(hdr.split(f"#define {name}")[1].split()[0].rstrip("u")) == val, name


def test_emu_known_answers(emu):
    check_known_answers(emu)


@pytest.mark.parametrize("small", [0, 1, 2], ids=["wave_per_entry", "four_per_wave", "eight_per_wave"])
def test_emu_every_length_and_phase(emu, small):
    check_every_length_and_phase(emu, small)


@pytest.mark.parametrize("small", [0, 1, 2], ids=["wave_per_entry", "four_per_wave", "eight_per_wave"])
def test_emu_random_lengths(emu, small):
    check_random_lengths(emu, small)


def test_emu_stream(emu):
    check_stream(emu)


@pytest.mark.parametrize("small", [0, 1, 2], ids=["wave_per_entry", "four_per_wave", "eight_per_wave"])
def test_emu_build_cases(emu, small):
    check_build_cases(emu, small)


@pytest.mark.parametrize("small", [0, 1, 2], ids=["wave_per_entry", "four_per_wave", "eight_per_wave"])
def test_emu_build_every_phase(emu, small):
    check_build_every_phase(emu, small)


# rgb_seg_combine_kernel alone: its rounds behind the first run only with more than 256 partial values, a buffer of more
# than 16 MiB -- too long for the fibers (the GPU's 64 MiB lengths of check_stream stay).  tests/native exports the
# kernel on given partial values; the referee is the same polynomial sum in Python.

POLY = 0xEDB88320              # reflected: x^k is bit 31 - k


def gf2_mulmod(a: int, b: int) -> int:
    """a * b mod P over GF(2), both in the reflected representation (zlib's multmodp)"""
    p, m = 0, 1 << 31
    while m:
        if a & m:
            p ^= b
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
        m >>= 1
    return p


def gf2_xpow8(n: int) -> int:
    """x^(8 n) mod P"""
    p, sq = 1 << 31, 1 << 23
    while n:
        if n & 1:
            p = gf2_mulmod(sq, p)
        sq, n = gf2_mulmod(sq, sq), n >> 1
    return p


def raw_crc(m: bytes) -> int:
    """M(x) x^32 mod P, from zlib: crc(M, init) = ~( ~init x^(8 |M|) ^ raw(M) )  (rgb_segment.hip, "the arithmetic")"""
    return (~zlib.crc32(m, 0) & 0xFFFFFFFF) ^ gf2_mulmod(0xFFFFFFFF, gf2_xpow8(len(m)))


def combine_in_python(partials, xn, start):
    raw, xblk = 0, gf2_xpow8(STREAM_BLOCK)
    for p in partials:                                      # Horner: raw = xor_b partials[b] x^(8 STREAM_BLOCK (n - 1 - b))
        raw = gf2_mulmod(raw, xblk) ^ int(p)
    return ~(gf2_mulmod(~start & 0xFFFFFFFF, xn) ^ raw) & 0xFFFFFFFF


def test_gf2_referee_against_zlib():
    """The Python arithmetic pinned first: raw(A ++ B) = raw(A) x^(8 |B|) ^ raw(B) and crc(M, init) as the kernel's
    comment states them, with zlib.crc32 on both sides; and the combine sum itself on a buffer of three blocks."""
    rng = np.random.default_rng(370)
    assert gf2_mulmod(1 << 31, 0x12345678) == 0x12345678 and gf2_xpow8(0) == 1 << 31
    for la, lb in ((0, 5), (1, 1), (17, 4096), (STREAM_BLOCK, 3), (70001, 2 * STREAM_BLOCK)):
        a, b = rng.bytes(la), rng.bytes(lb)
        assert raw_crc(a + b) == gf2_mulmod(raw_crc(a), gf2_xpow8(lb)) ^ raw_crc(b), (la, lb)
        init = int(rng.integers(0, 1 << 32))
        assert zlib.crc32(b, init) == ~(gf2_mulmod(~init & 0xFFFFFFFF, gf2_xpow8(lb)) ^ raw_crc(b)) & 0xFFFFFFFF
    m = rng.bytes(2 * STREAM_BLOCK + 77)                    # blocks aligned to the END: the first one is the short one
    parts = [raw_crc(m[:77]), raw_crc(m[77:77 + STREAM_BLOCK]), raw_crc(m[77 + STREAM_BLOCK:])]
    assert combine_in_python(parts, gf2_xpow8(len(m)), 0x1234) == zlib.crc32(m, 0x1234)


COMBINE_BLOCKS = [1, 2, 255, 256, 257, 511, 512, 513, 1000]


@pytest.mark.parametrize("n_blocks", COMBINE_BLOCKS)
def test_emu_combine_rounds(emu, n_blocks):
    import ctypes as C
    fn = emu.engine.lib().emu_seg_combine
    fn.restype, fn.argtypes = C.c_uint32, [C.c_void_p] + [C.c_uint32] * 5
    rng = np.random.default_rng(380 + n_blocks)
    partials = rng.integers(0, 1 << 32, size=n_blocks, dtype=np.uint32)
    xn, init, held = (int(x) for x in rng.integers(1, 1 << 32, size=3))
    # the two forms of the starting value: the argument, or what *crc holds (the next gigabyte of one buffer)
    assert fn(partials.ctypes.data, n_blocks, xn, init, 0, held) == combine_in_python(partials, xn, init)
    assert fn(partials.ctypes.data, n_blocks, xn, init, 1, held) == combine_in_python(partials, xn, held)


def test_emu_refusals(emu):
    check_refusals(emu)


def test_emu_round_trip(emu):
    check_round_trip(emu)


@pytest.mark.parametrize("sched", PERMUTED_SCHEDULES)
def test_emu_under_permuted_schedules(emu, sched):
    """The emulation's own order is workgroups 0, 1, 2, ... and lanes 0 .. 255.  The build cases (every lane-group
    width), the stream CRC (its partial values are joined by a later launch) and the round trip with workgroups and lanes
    reversed and permuted (tests/emu_schedule.py); the referee stays zlib and struct.pack."""
    with schedule(emu.engine, sched):
        for small in (0, 1, 2):
            check_build_cases(emu, small)
        check_stream(emu)
        check_round_trip(emu)


def test_segment_scan_under_sanitizers(tmp_path):
    """rgb_segment_scan compiled with AddressSanitizer + UBSan (host-only translation unit, plain g++) over 300
    damaged and truncated images, each in an exactly-sized heap block; the harness prints rc, count, version,
    MaxCount and end reason, compared with a walk written here."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "segment_scan_harness"
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-o", str(exe),
           os.path.join(ROOT, "tests", "native", "segment_scan_harness.cpp"),
           os.path.join(ROOT, "ra_amd", "csrc", "rgb_segment_host.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert built.returncode == 0, built.stderr

    def walk(f: bytes):
        if len(f) < 8 or f[:4] != b"RASG":
            return (E_INVAL, 0, 0, 0, 0)
        version, mc = struct.unpack(">HH", f[4:8])
        if version not in (1, 2):
            return (E_INVAL, 0, 0, 0, 0)
        rec, fmt = (32, ">QQQII") if version == 2 else (28, ">QQIII")
        n = 0
        for k in range(mc):
            pos = 8 + rec * k
            if pos + rec > len(f):
                return (0, n, version, mc, abi.SEG_END_TRUNCATED)
            idx, term, off, ln, crc = struct.unpack(fmt, f[pos:pos + rec])
            if (idx, term, off, ln, crc) == (0, 0, 0, 0, 0):
                return (0, n, version, mc, abi.SEG_END_ZEROS)
            if off + ln > len(f):
                return (0, n, version, mc, abi.SEG_END_TRUNCATED)
            n += 1
        return (0, n, version, mc, abi.SEG_END_FULL)

    rng = np.random.default_rng(78)
    lens = [int(x) for x in rng.integers(0, 400, size=30)]
    payloads = [rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes() for ln in lens]
    files, want = [], []
    for trial in range(300):
        version = 1 + trial % 2
        f = bytearray(python_segment([(i + 1, 3) for i in range(30)], payloads, 30 + trial % 3, version=version))
        r = rng.random()
        if r < 0.4:
            for _ in range(int(rng.integers(1, 6))):
                f[int(rng.integers(4, len(f)))] = int(rng.integers(0, 256))
        elif r < 0.8:
            del f[int(rng.integers(0, len(f))):]
        else:
            f = f[:int(rng.integers(8, len(f)))] + bytes(rng.integers(0, 256, size=int(rng.integers(0, 80)), dtype=np.uint8))
        path = tmp_path / f"s{trial}.segment"
        path.write_bytes(bytes(f))
        files.append(str(path))
        want.append(walk(bytes(f)))
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in run.stdout.splitlines()]
    assert got == want


def test_new_kernels_use_no_scratch():
    """hipcc's resource remarks for gfx950 (no GPU needed), as tests/test_kernel_resources.py reads them: every
    kernel of rgb_segment.hip without scratch or spills, 20 KiB of LDS, at least 7 wavefronts per SIMD."""
    from test_kernel_resources import segment_usage
    usage = segment_usage()
    names = [k for k in usage if "rgb_seg_" in k]
    assert len(names) == 8, names                       # 3 widths x {crc, build}, stream, combine
    for k in names:
        u = usage[k]
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, f"{k}: {u}"
        assert u["Occupancy"] >= 7 and u["LDS Size"] <= 20 * 1024 + 64, f"{k}: {u}"


# ------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
def test_gpu_known_answers(gpu):
    check_known_answers(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("small", [0, 1, 2], ids=["wave_per_entry", "four_per_wave", "eight_per_wave"])
def test_gpu_every_length_and_phase(gpu, small):
    check_every_length_and_phase(gpu, small)


@pytest.mark.gpu
@pytest.mark.parametrize("small", [0, 1, 2], ids=["wave_per_entry", "four_per_wave", "eight_per_wave"])
def test_gpu_random_lengths(gpu, small):
    check_random_lengths(gpu, small)


@pytest.mark.gpu
def test_gpu_stream(gpu):
    check_stream(gpu)


@pytest.mark.gpu
def test_gpu_stream_64_mib(gpu):
    import torch
    n = 64 << 20
    t = torch.randint(0, 256, (n + 16,), dtype=torch.uint8, device="cuda")
    host = t.cpu().numpy()
    d_c = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for phase, ln, init in ((0, n, 0), (3, n - 1, 0x1234ABCD)):
        gpu.eng.crc32_stream_device(t.data_ptr() + phase, ln, init, d_c.data_ptr())
        gpu.eng.synchronize()
        got = int(d_c.cpu().numpy().view(np.uint32)[0])
        assert got == zlib.crc32(host[phase:phase + ln].tobytes(), init), (phase, ln)


@pytest.mark.gpu
@pytest.mark.parametrize("small", [0, 1, 2], ids=["wave_per_entry", "four_per_wave", "eight_per_wave"])
def test_gpu_build_cases(gpu, small):
    check_build_cases(gpu, small)


@pytest.mark.gpu
@pytest.mark.parametrize("small", [0, 1, 2], ids=["wave_per_entry", "four_per_wave", "eight_per_wave"])
def test_gpu_build_every_phase(gpu, small):
    check_build_every_phase(gpu, small)


@pytest.mark.gpu
def test_gpu_refusals(gpu):
    check_refusals(gpu)


@pytest.mark.gpu
def test_gpu_round_trip(gpu):
    check_round_trip(gpu)


@pytest.mark.gpu
def test_gpu_full_size_segment(gpu):
    """4096 entries of 40 B .. 256 KiB (log-uniform, so that the image stays inside ?SEGMENT_MAX_SIZE_B), built on
    the device, read back and compared whole."""
    rng = np.random.default_rng(370)
    lens = np.exp(rng.uniform(np.log(40), np.log(256 * 1024), size=4096)).astype(np.int64)
    lens[:4] = (40, 256 * 1024, 41, 256 * 1024 - 1)
    while 8 + 32 * 4096 + int(lens.sum()) > abi.SEG_MAX_SIZE_B - 65536:
        lens[int(np.argmax(lens[4:])) + 4] = 40
    entries, data, payloads = pack_entries(rng, [int(x) for x in lens])
    want = python_segment([(int(e["index"]), int(e["term"])) for e in entries], payloads, 4096)
    assert len(want) <= abi.SEG_MAX_SIZE_B
    got, behind = device_build(gpu, entries, data, 4096, 0, 5, 11)
    assert first_diff(got, want) is None, first_diff(got, want)
    assert np.all(behind == 0xEE)
    recs = gpu.engine.segment_scan(np.frombuffer(got, dtype=np.uint8))[0]
    assert len(recs) == 4096 and gpu.eng.segment_validate(np.frombuffer(got, dtype=np.uint8), recs) == 4096
