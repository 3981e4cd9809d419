"""WAL entry checksums (include/ra_gpu_wal.h): the CPU checker against
the published Adler-32 vectors and zlib, the HIP kernel against both."""
import struct
import time
import zlib

import numpy as np
import pytest

from ra_amd import abi
from oracle import oracle as O


def frame(index, term, payload: bytes) -> bytes:
    """Entry = [<<Idx:64/unsigned, Term:64/unsigned>> | EntryData]  (src/ra_log_wal.erl:528-530)"""
    return struct.pack(">QQ", index, term) + payload


def _engine():
    import os
    from ra_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build()
    return engine


FAMILIES = ("random", "ff", "zero", "ff_one_zero")
ADLER_MOD = 65521
EDGE_LENS = [0, 1, 15, 16, 17, 5551, 5552, 5553, 65520, 65521, 65522, 1 << 20]   # chunk, zlib's NMAX, the modulus
MIB = 1 << 20


def family_bytes(rng, family, n) -> np.ndarray:
    """n payload bytes: uniform random, the worst case for the sums (all 0xFF), all zero, 0xFF with one 0x00."""
    if family == "random":
        return rng.integers(0, 256, size=n, dtype=np.uint8)
    out = np.full(n, 0x00 if family == "zero" else 0xFF, dtype=np.uint8)
    if family == "ff_one_zero" and n:
        out[int(rng.integers(0, n))] = 0
    return out


def make_batch(rng, lens, misalign=True, family="random"):
    """Payloads packed back to back (arbitrary alignment) into one buffer, 16 spare bytes behind."""
    entries = np.zeros(len(lens), dtype=abi.WAL_ENTRY_DTYPE)
    off = int(rng.integers(0, 16)) if misalign else 0
    chunks = []
    pos = 0
    for i, ln in enumerate(lens):
        pad = int(rng.integers(0, 5)) if misalign else (-pos) % 16
        chunks.append(bytes(pad)); pos += pad
        entries["index"][i] = int(rng.integers(0, 1 << 62))
        entries["term"][i] = int(rng.integers(0, 1 << 40))
        entries["data_offset"][i] = off + pos
        entries["data_len"][i] = ln
        chunks.append(family_bytes(rng, family, ln).tobytes()); pos += ln
    data = np.frombuffer(bytes(off) + b"".join(chunks) + bytes(32), dtype=np.uint8).copy()
    return entries, data


def width_batch(rng, lens, family, width):
    """make_batch plus what makes rgb_wal_adler32_device take `width` lanes per entry: 16 below a mean of 1 KiB
    (empty entries are added), a wavefront otherwise (the buffer is lengthened)."""
    entries, data = make_batch(rng, lens, True, family)
    if width == 16:
        more = np.zeros(len(data) // 1024 + 1, dtype=abi.WAL_ENTRY_DTYPE)
        more["index"], more["term"] = np.arange(len(more)) + 7, 3
        entries = np.concatenate([entries, more])
    elif len(data) < 1024 * len(entries):
        data = np.concatenate([data, np.zeros(1024 * len(entries) - len(data), dtype=np.uint8)])
    assert (len(data) // len(entries) < 1024) == (width == 16)
    return entries, data


def chunk_sums(stream: np.ndarray):
    """(a, b) of every 16-byte chunk of `stream` (a multiple of 16 bytes), exact: a = sum d_j, b = sum (16 - j) d_j"""
    a, b = np.zeros(len(stream) // 16, dtype=np.uint64), np.zeros(len(stream) // 16, dtype=np.uint64)
    weights = np.arange(16, 0, -1, dtype=np.uint32)
    step = 1 << 20                                                     # chunks per slice: 64 MiB of uint32 at a time
    for c0 in range(0, len(a), step):
        x = stream[16 * c0:16 * (c0 + step)].reshape(-1, 16).astype(np.uint32)
        a[c0:c0 + step] = x.sum(axis=1)
        b[c0:c0 + step] = x @ weights
    return a, b


def unfolded_lane_sums(stream: np.ndarray, weight_of_first: int, group: int):
    """What the lanes of a group would hold WITHOUT the folds at WAL_FOLD_AT, in exact 64-bit arithmetic: chunk c of
    `stream` goes to lane c mod group and adds a_c to the lane's a_acc and (wq a_c + b_c) mod 65521 to its b_acc,
    wq = (W - 16 c - 16) mod 65521 with W the weight of the stream's first byte.  -> (a sums, b sums) per lane."""
    a, b = chunk_sums(stream)
    c = np.arange(len(a), dtype=np.int64)
    wq = ((weight_of_first - 16 * c - 16) % ADLER_MOD).astype(np.uint64)
    term = (wq * a + b) % np.uint64(ADLER_MOD)
    pad = (-len(a)) % group
    a, term = np.concatenate([a, np.zeros(pad, dtype=np.uint64)]), np.concatenate([term, np.zeros(pad, dtype=np.uint64)])
    return a.reshape(-1, group).sum(axis=0), term.reshape(-1, group).sum(axis=0)


def zlib_checksums(entries, data):
    out = np.zeros(len(entries), dtype=np.uint32)
    for i, e in enumerate(entries):
        o, n = int(e["data_offset"]), int(e["data_len"])
        out[i] = zlib.adler32(frame(int(e["index"]), int(e["term"]), data[o:o + n].tobytes()))
    return out


def test_oracle_adler32_known_answers():
    assert O.adler32(b"") == 1                                   # RFC 1950: s1 = 1, s2 = 0
    assert O.adler32(b"Wikipedia") == 0x11E60398                 # the textbook vector
    assert O.adler32(b"a") == 0x00620062
    assert O.adler32(bytes(range(256)) * 300) == zlib.adler32(bytes(range(256)) * 300)  # wraps 65521 often


def test_oracle_wal_entry_checksum_matches_zlib():
    rng = np.random.default_rng(7)
    lens = [0, 1, 15, 16, 17, 255, 4096, 70001] + [int(x) for x in rng.integers(0, 3000, size=40)]
    entries, data = make_batch(rng, lens)
    assert np.array_equal(O.wal_entry_checksums(entries, data), zlib_checksums(entries, data))
    # the reference's validation is the same function on the read path (src/ra_log_wal.erl:861)
    e0 = entries[3]
    payload = data[int(e0["data_offset"]):int(e0["data_offset"]) + int(e0["data_len"])].tobytes()
    assert O.wal_entry_checksums(entries[3:4], data)[0] == zlib.adler32(frame(int(e0["index"]), int(e0["term"]), payload))


def test_oracle_detects_overwritten_bytes():
    """test/ra_log_wal_SUITE.erl:1500-1528 checksum_failure_in_middle_of_file_should_fail: 1000-byte
    entries, ten bytes of one record overwritten with zeros -> validation must fail for that record
    (and only for it)."""
    rng = np.random.default_rng(3)
    entries, data = make_batch(rng, [1000] * 100, misalign=False)
    entries["term"] = 1
    entries["index"] = np.arange(1, 101)
    stored = O.wal_entry_checksums(entries, data)
    victim = 42
    o = int(entries["data_offset"][victim])
    data[o + 500:o + 510] = np.where(data[o + 500:o + 510] == 0, 1, 0)     # guaranteed to differ
    again = O.wal_entry_checksums(entries, data)
    assert again[victim] != stored[victim]
    assert np.array_equal(np.delete(again, victim), np.delete(stored, victim))


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [True, False])
def test_gpu_wal_checksums_match_oracle_and_zlib(misalign):
    import torch
    engine = _engine()
    rng = np.random.default_rng(11 + misalign)
    lens = [0, 1, 2, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 70001,
            1 << 20] + [int(x) for x in rng.integers(0, 20000, size=300)]
    entries, data = make_batch(rng, lens, misalign)
    eng = engine.RaGpuBatch(1, 1)
    d_e = torch.from_numpy(entries.view(np.uint8)).cuda()
    d_d = torch.from_numpy(data).cuda()
    d_o = torch.zeros(len(entries), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                  # the library launches on its own stream
    eng.wal_adler32_device(d_e.data_ptr(), len(entries), d_d.data_ptr(), len(data), d_o.data_ptr())
    torch.cuda.synchronize()
    got = d_o.cpu().numpy().view(np.uint32)
    want = O.wal_entry_checksums(entries, data)
    assert np.array_equal(want, zlib_checksums(entries, data))
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"entry {bad[0]} len {lens[bad[0]]}: gpu {got[bad[0]]:#x} oracle {want[bad[0]]:#x}"
    eng.close()


@pytest.mark.gpu
def test_gpu_wal_host_buffer_form():
    """rgb_wal_adler32: host buffers in, host checksums out (what the NIF binds); grows its staging."""
    engine = _engine()
    rng = np.random.default_rng(31)
    eng = engine.RaGpuBatch(1, 1)
    for lens in ([0, 5, 100, 4096], [int(x) for x in rng.integers(0, 9000, size=500)], [1 << 20, 3]):
        entries, data = make_batch(rng, lens, True)
        assert np.array_equal(eng.wal_adler32(entries, data), zlib_checksums(entries, data))
    bad = np.zeros(1, dtype=abi.WAL_ENTRY_DTYPE)
    bad["data_offset"] = 10; bad["data_len"] = 100
    with pytest.raises(engine.RgbError):
        eng.wal_adler32(bad, np.zeros(50, dtype=np.uint8))          # payload outside the buffer
    eng.close()


@pytest.mark.gpu
def test_gpu_wal_checksums_small_entries():
    """Mean payload below 1 KiB: the four-entries-per-wavefront variant."""
    import torch
    engine = _engine()
    rng = np.random.default_rng(23)
    lens = [0, 1, 15, 16, 17, 240, 255, 256, 257, 1023] + [int(x) for x in rng.integers(0, 700, size=1013)]
    entries, data = make_batch(rng, lens, True)
    assert len(data) / len(lens) < 1024
    eng = engine.RaGpuBatch(1, 1)
    d_e = torch.from_numpy(entries.view(np.uint8)).cuda()
    d_d = torch.from_numpy(data).cuda()
    d_o = torch.zeros(len(entries), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.wal_adler32_device(d_e.data_ptr(), len(entries), d_d.data_ptr(), len(data), d_o.data_ptr())
    torch.cuda.synchronize()
    got = d_o.cpu().numpy().view(np.uint32)
    want = zlib_checksums(entries, data)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"entry {bad[0]} len {lens[bad[0]]}: gpu {got[bad[0]]:#x} zlib {want[bad[0]]:#x}"
    eng.close()


@pytest.mark.gpu
def test_gpu_wal_checksums_full_size_properties():
    """4 GiB-class batches cannot be checked byte by byte on the CPU in seconds: check the property
    Adler-32 offers -- the checksum of a record is a function of (A, B) sums that are additive, so
    flipping one byte by +1 at position p from the end changes A by 1 and B by p (mod 65521)."""
    import torch
    engine = _engine()
    rng = np.random.default_rng(5)
    n, ln = 4096, 65536
    entries = np.zeros(n, dtype=abi.WAL_ENTRY_DTYPE)
    entries["index"] = np.arange(n); entries["term"] = 7
    entries["data_offset"] = np.arange(n, dtype=np.uint64) * ln
    entries["data_len"] = ln
    data = rng.integers(0, 255, size=n * ln + 16, dtype=np.uint8)      # < 255 so +1 never wraps a byte
    eng = engine.RaGpuBatch(1, 1)
    d_e = torch.from_numpy(entries.view(np.uint8)).cuda()
    d_d = torch.from_numpy(data).cuda()
    d_o = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                  # the library launches on its own stream
    eng.wal_adler32_device(d_e.data_ptr(), n, d_d.data_ptr(), len(data), d_o.data_ptr())
    torch.cuda.synchronize()
    before = d_o.cpu().numpy().view(np.uint32).copy()
    # spot-check a sample against the CPU
    sample = rng.choice(n, size=24, replace=False)
    assert np.array_equal(before[sample], O.wal_entry_checksums(entries[sample], data))
    pos = rng.integers(0, ln, size=n)                                    # byte position inside each record
    flat = torch.from_numpy((np.arange(n, dtype=np.int64) * ln + pos)).cuda()
    d_d[flat] += 1
    torch.cuda.synchronize()
    eng.wal_adler32_device(d_e.data_ptr(), n, d_d.data_ptr(), len(data), d_o.data_ptr())
    torch.cuda.synchronize()
    after = d_o.cpu().numpy().view(np.uint32)
    a0, b0 = before & 0xFFFF, before >> 16
    a1, b1 = after & 0xFFFF, after >> 16
    assert np.array_equal((a0.astype(np.int64) + 1) % 65521, a1)
    assert np.array_equal((b0.astype(np.int64) + (ln - pos)) % 65521, b1)
    eng.close()


# ---- payloads that are not uniformly random, and the accumulator folds -----------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES[1:])
@pytest.mark.parametrize("width", [16, 64])
def test_gpu_wal_checksums_payload_families(width, family):
    """All 0xFF (the largest sums a length can give), all zero, 0xFF with one zero: both lane widths."""
    import torch
    engine = _engine()
    rng = np.random.default_rng(400 + width + FAMILIES.index(family))
    entries, data = width_batch(rng, EDGE_LENS, family, width)
    eng = engine.RaGpuBatch(1, 1)
    d_e, d_d = torch.from_numpy(entries.view(np.uint8)).cuda(), torch.from_numpy(data).cuda()
    d_o = torch.zeros(len(entries), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.wal_adler32_device(d_e.data_ptr(), len(entries), d_d.data_ptr(), len(data), d_o.data_ptr())
    torch.cuda.synchronize()
    got, want = d_o.cpu().numpy().view(np.uint32), zlib_checksums(entries, data)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"entry {bad[0]} len {int(entries['data_len'][bad[0]])}: gpu {got[bad[0]]:#x} zlib {want[bad[0]]:#x}"
    eng.close()


class FoldRun:
    """One context for the cases of a module that reach WAL_FOLD_AT = 0x7FFF0000 of rgb_wal.hip, one launch per case on
    a stream of the test's own, each waited for under its own time limit.  A launch that does not end in time fails its
    case, and every later case of this object fails without launching.  That is all this guard can do: the buffers of
    the stuck launch are kept alive here (not handed back while a kernel may still use them) and the context stays
    open, but tests of other modules in the same session are not held back."""
    LIMIT_S = 60.0

    def __init__(self):
        import torch
        self.torch, self.engine = torch, _engine()
        self.eng = self.engine.RaGpuBatch(1, 1)
        self.stream = torch.cuda.Stream()
        self.stuck, self.parked = False, []

    def launch(self, enqueue, buffers):
        """enqueue(stream handle) over the device `buffers` -> seconds until the stream was idle again"""
        torch = self.torch
        assert not self.stuck, "an earlier launch of this module did not end: no further launch from here"
        torch.cuda.synchronize()                               # the inputs came through torch's own stream
        done = torch.cuda.Event()
        t0 = time.perf_counter()
        enqueue(self.stream.cuda_stream)
        done.record(self.stream)
        while not done.query():
            if time.perf_counter() - t0 > self.LIMIT_S:
                self.stuck = True
                self.parked += list(buffers)
                pytest.fail(f"the launch did not end within {self.LIMIT_S} s")
        return time.perf_counter() - t0

    def close(self):
        if not self.stuck:
            self.eng.close()


@pytest.fixture(scope="module")
def fold_run():
    run = FoldRun()
    yield run
    run.close()


# (lanes per entry, payload bytes, family, empty entries beside it, the sum that has to pass 2^32)
ADLER_FOLD_CASES = {"b_16_lanes": (16, 64 * MIB, "random", 65537, "b"),
                    "b_64_lanes": (64, 256 * MIB, "random", 0, "b"),
                    "a_16_lanes": (16, 272 * MIB, "ff", 278529, "a")}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ADLER_FOLD_CASES))
def test_gpu_adler_folds_at_the_real_threshold(fold_run, case):
    """A lane's b_acc passes WAL_FOLD_AT after about 65 000 chunks and a_acc after 526 000 chunks of 0xFF, so only one
    long entry reaches the folds: 2^18 random chunks per lane for b_acc, 2^20 + 2^16 chunks of 0xFF per lane for a_acc
    (the narrowest group only: the widths share the line).  Before anything is launched the sums a lane would form
    WITHOUT folding are computed exactly; one of them has to exceed 2^32, or the input no longer tests the fold (the
    dispatch limits or the lane mapping have changed).  Referee: zlib.adler32."""
    torch = fold_run.torch
    lanes, n_bytes, family, empties, which = ADLER_FOLD_CASES[case]
    rng = np.random.default_rng(700 + lanes)
    lead = 5                                                   # the entry starts 5 bytes into a 16-byte chunk
    payload = np.frombuffer(rng.bytes(n_bytes), dtype=np.uint8) if family == "random" else family_bytes(rng, family, n_bytes)
    data = np.concatenate([np.zeros(lead, dtype=np.uint8), payload, np.zeros(16, dtype=np.uint8)])   # 16 spare bytes
    entries = np.zeros(1 + empties, dtype=abi.WAL_ENTRY_DTYPE)
    entries["index"], entries["term"] = np.arange(len(entries)) + (1 << 40), 9
    entries["data_offset"][0], entries["data_len"][0] = lead, n_bytes
    assert (len(data) // len(entries) < 1024) == (lanes == 16)
    span = lead + n_bytes
    stream = np.concatenate([data[:span], np.zeros((-span) % 16, dtype=np.uint8)])
    a_sums, b_sums = unfolded_lane_sums(stream, span, lanes)
    top = int((a_sums if which == "a" else b_sums).max())
    print(f"{case}: largest unfolded {which}_acc of a lane {top} = 2^32 * {top / 2 ** 32:.3f}")
    assert top > 2 ** 32, "no lane's sum passes 2^32: this input does not reach the fold"
    want = zlib.adler32(payload, zlib.adler32(struct.pack(">QQ", int(entries["index"][0]), 9)))
    d_e, d_d = torch.from_numpy(entries.view(np.uint8)).cuda(), torch.from_numpy(data).cuda()
    d_o = torch.zeros(len(entries), dtype=torch.int32, device="cuda")
    took = fold_run.launch(lambda st: fold_run.eng.wal_adler32_device(d_e.data_ptr(), len(entries), d_d.data_ptr(),
                                                                      len(data), d_o.data_ptr(), st),
                           (d_e, d_d, d_o))
    print(f"{case}: kernel {took * 1e3:.1f} ms")
    got = d_o.cpu().numpy().view(np.uint32)
    assert int(got[0]) == want, f"{case}: gpu {int(got[0]):#x} zlib {want:#x}"
    if empties:                                                # the empty entries beside it: the 16 framed bytes alone
        for i in (1, empties // 2, empties):
            assert int(got[i]) == zlib.adler32(frame(int(entries["index"][i]), 9, b"")), i
