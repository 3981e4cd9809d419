#!/usr/bin/env python3
"""Rates of major compaction on the device (include/ra_gpu_wal.h: rgb_segment_compact_device, with and without
RGB_SEG_COMPACT_VERIFY), device-resident forms, HIP events around 20 calls after 3 warm-up calls, five repeats.
A compaction group is 4 source segments of 4096 entries each, a quarter of the entries live (four consecutive indexes
out of every sixteen), at 256 B, 4 KiB and 64 KiB payloads: the new segment has 4096 entries.  Timed in the same run, on
the same live payloads: (a) rgb_segment_build_device over them laid out contiguously -- CRC and copy, what a flush of
the same entries costs; (b) a device-to-device copy of the same byte count.  Before anything is timed the image is
compared (max_size is raised to 512 MB: 4096 live entries of 64 KiB exceed the default) with one put together by numpy from the source bytes, and for the 256 B group with the sequential referee of
tests/test_segment_compact.py.  Writes its rows as JSON to profiles/segment_compact_bench.json (or argv[1])."""
import json, os, struct, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from ra_amd import abi, engine

assert torch.cuda.is_available(), "segment_compact_bench.py measures on the GPU; there is no CPU fallback"
eng = engine.RaGpuBatch(1, 1)
stream = torch.cuda.Stream(); sp = stream.cuda_stream
REPS, WARM, REPEATS = 20, 3, 5
N_SOURCES, PER_SOURCE = 4, 4096
REC = np.dtype([("idx", ">u8"), ("term", ">u8"), ("off", ">u8"), ("len", ">u4"), ("crc", ">u4")])


def timed(fn):
    """us per call: (median, min, max) over REPEATS measurements of REPS calls"""
    out = []
    for _ in range(REPEATS):
        with torch.cuda.stream(stream):
            for _ in range(WARM):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(REPS):
                fn()
            e1.record(stream)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / REPS)
    return float(np.median(out)), float(min(out)), float(max(out))


res = []
for label, size in (("256 B entries", 256), ("4 KiB entries", 4096), ("64 KiB entries", 65536)):
    data_start = 8 + 32 * PER_SOURCE
    file_bytes = data_start + PER_SOURCE * size
    total = N_SOURCES * file_bytes
    d_files = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
    host = d_files.cpu().numpy()
    sources = np.zeros(N_SOURCES, dtype=abi.SEG_SOURCE_DTYPE)
    live = []
    for s in range(N_SOURCES):
        first = 1 + s * PER_SOURCE
        index = np.zeros(PER_SOURCE, dtype=REC)
        index["idx"] = np.arange(first, first + PER_SOURCE); index["term"] = 7
        index["off"] = data_start + np.arange(PER_SOURCE, dtype=np.uint64) * size
        index["len"] = size
        for k in range(PER_SOURCE):                         # the live records carry their Crc, the others 0 ("not checked")
            if k % 16 < 4:
                at = s * file_bytes + data_start + k * size
                index["crc"][k] = zlib.crc32(host[at:at + size])
        head = np.frombuffer(struct.pack(">4sHH", b"RASG", 2, PER_SOURCE) + index.tobytes(), dtype=np.uint8)
        host[s * file_bytes:s * file_bytes + data_start] = head
        d_files[s * file_bytes:s * file_bytes + data_start] = torch.from_numpy(head.copy()).cuda()
        sources["offset"][s], sources["n_bytes"][s] = s * file_bytes, file_bytes
        sources["live_first"][s], sources["live_n"][s] = len(live), PER_SOURCE // 16
        live += [(first + 16 * k, first + 16 * k + 3) for k in range(PER_SOURCE // 16)]
    live = np.array(live, dtype=np.uint64)
    bound, max_count = engine.segment_compact_bound(sources, live, total)
    assert max_count == N_SOURCES * PER_SOURCE // 4
    live_bytes = max_count * size
    image_bytes = 8 + 32 * max_count + live_bytes
    d_out = torch.zeros(image_bytes, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    # the expected image, by numpy: which records are live, their index records with new offsets, their payloads
    pos = np.concatenate([np.arange(int(a), int(b) + 1, dtype=np.int64) for a, b in live]) - 1      # record number over all sources
    src_of, rec_of = pos // PER_SOURCE, pos % PER_SOURCE
    want_index = np.zeros(max_count, dtype=REC)
    want_index["idx"] = pos + 1; want_index["term"] = 7; want_index["len"] = size
    want_index["crc"] = [zlib.crc32(host[a:a + size]) for a in src_of * file_bytes + data_start + rec_of * size]
    want_index["off"] = 8 + 32 * max_count + np.arange(max_count, dtype=np.uint64) * size
    payload_at = src_of * file_bytes + data_start + rec_of * size
    want = np.concatenate([np.frombuffer(struct.pack(">4sHH", b"RASG", 2, max_count) + want_index.tobytes(), dtype=np.uint8),
                           ] + [host[a:a + size] for a in payload_at])
    for flags in (0, abi.SEG_COMPACT_VERIFY):
        d_out.zero_()
        torch.cuda.synchronize()
        eng.segment_compact_device(sources, d_files.data_ptr(), total, live, d_out.data_ptr(), image_bytes,
                                   d_res.data_ptr(), abi.SEG_MAX_SIZE_B * 8, flags, sp)
        eng.synchronize(); torch.cuda.synchronize()
        r = d_res.cpu().numpy().view(abi.SEG_COMPACT_RESULT_DTYPE)[0]
        assert (int(r["status"]), int(r["n_entries"]), int(r["file_bytes"])) == (0, max_count, image_bytes), (label, r)
        assert np.array_equal(d_out.cpu().numpy(), want), f"{label}, flags {flags}: the image differs"
    if size == 256:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_segment_compact import ref_compact
        files = [host[s * file_bytes:(s + 1) * file_bytes].tobytes() for s in range(N_SOURCES)]
        lives = [[tuple(int(x) for x in p) for p in live[int(sources["live_first"][s]):][:int(sources["live_n"][s])]]
                 for s in range(N_SOURCES)]
        assert ref_compact(files, lives) == want.tobytes(), "the numpy image differs from the referee's"

    def compact(flags):
        return lambda: eng.segment_compact_device(sources, d_files.data_ptr(), total, live, d_out.data_ptr(), image_bytes,
                                                  d_res.data_ptr(), abi.SEG_MAX_SIZE_B * 8, flags, sp)
    plain, verify = timed(compact(0)), timed(compact(abi.SEG_COMPACT_VERIFY))

    # (a) rgb_segment_build_device over the same live payloads, contiguous
    d_live = torch.from_numpy(want[8 + 32 * max_count:].copy()).cuda()
    ents = np.zeros(max_count, dtype=abi.SEG_ENTRY_DTYPE)
    ents["index"] = pos + 1; ents["term"] = 7; ents["data_len"] = size
    ents["data_offset"] = np.arange(max_count, dtype=np.uint64) * size
    offs_out, size_out = engine.segment_layout(ents, max_count)
    assert size_out == image_bytes
    d_e = torch.from_numpy(ents.view(np.uint8)).cuda()
    d_f = torch.from_numpy(offs_out.view(np.uint8)).cuda()
    d_b = torch.zeros(size_out, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    build = timed(lambda: eng.segment_build_device(d_e.data_ptr(), max_count, max_count, d_f.data_ptr(), d_live.data_ptr(),
                                                   live_bytes, d_b.data_ptr(), size_out, 0, sp))
    assert np.array_equal(d_b[8 + 32 * max_count:].cpu().numpy(), want[8 + 32 * max_count:])
    # (b) a device-to-device copy of the same byte count
    d_c = torch.empty(live_bytes, dtype=torch.uint8, device="cuda")
    memcpy = timed(lambda: d_c.copy_(d_live, non_blocking=True))

    gb = live_bytes / 1e9
    row = {"workload": label, "sources": N_SOURCES, "entries_per_source": PER_SOURCE, "live_entries": int(max_count),
           "live_payload_bytes": int(live_bytes), "source_bytes": int(total), "repeats": REPEATS, "calls_per_repeat": REPS}
    for name, (med, lo, hi) in (("compact", plain), ("compact_verify", verify), ("segment_build", build), ("memcpy_d2d", memcpy)):
        row[name + "_us"], row[name + "_us_min"], row[name + "_us_max"] = med, lo, hi
        row[name + "_GBps"] = gb / (med * 1e-6)
    for name in ("compact", "compact_verify"):
        row[name + "_vs_build"] = row["segment_build_us"] / row[name + "_us"]          # > 1: faster than the build
        row[name + "_vs_memcpy"] = row["memcpy_d2d_us"] / row[name + "_us"]
    res.append(row)
    print(json.dumps(row), flush=True)
    del d_files, d_out, d_live, d_b, d_c, d_e, d_f, host, want

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "segment_compact_bench.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
eng.close()
