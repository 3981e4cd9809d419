#!/usr/bin/env python3
"""Rates of the segment / snapshot CRC-32 kernels (include/ra_gpu_wal.h: rgb_crc32_device, rgb_segment_build_device,
rgb_crc32_stream_device), device-resident forms, HIP events around 20 launches after 3 warm-up launches.  Timed in the
same run: (a) zlib.crc32 over the same bytes on one host thread and on 16 (zlib releases the GIL) -- what the kernels
replace; (b) the project's rgb_wal_adler32_device / rgb_wal_frame_device on the same payloads -- the HBM-bound
yardstick for the same access pattern.  Every result is checked against zlib on a sample before it is timed.
Writes its rows as JSON to profiles/segment_bench.json (or argv[1])."""
import json, os, sys, time, zlib
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from ra_amd import abi, engine

assert torch.cuda.is_available(), "segment_bench.py measures on the GPU; there is no CPU fallback"
eng = engine.RaGpuBatch(1, 1)
stream = torch.cuda.Stream(); sp = stream.cuda_stream
REPS, WARM = 20, 3


def timed(fn):
    with torch.cuda.stream(stream):
        for _ in range(WARM):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(REPS):
            fn()
        e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS          # us per launch


def host_zlib(host, offs, lens, threads):
    """seconds for zlib.crc32 over every payload, split over `threads` host threads"""
    mv = memoryview(host)
    parts = np.array_split(np.arange(len(lens)), threads)

    def work(ix):
        for i in ix:
            zlib.crc32(mv[int(offs[i]):int(offs[i]) + int(lens[i])])
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        if threads == 1:
            work(parts[0])
        else:
            with ThreadPoolExecutor(threads) as ex:
                list(ex.map(work, parts))
        best = min(best, time.perf_counter() - t0)
    return best


res = []
TOTAL = 256 << 20                                     # payload bytes per batch
for label, size in (("256 B entries", 256), ("4 KiB entries", 4096), ("64 KiB entries", 65536)):
    n = TOTAL // size
    lens = np.full(n, size, dtype=np.uint32)
    offs = np.arange(n, dtype=np.uint64) * size
    ents = np.zeros(n, dtype=abi.SEG_ENTRY_DTYPE)
    ents["index"] = np.arange(1, n + 1); ents["term"] = 3; ents["data_offset"] = offs; ents["data_len"] = lens
    d_d = torch.randint(0, 256, (TOTAL + 16,), dtype=torch.uint8, device="cuda")
    host = d_d[:TOTAL].cpu().numpy()
    d_e = torch.from_numpy(ents.view(np.uint8)).cuda()
    d_c = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # per-entry CRC
    us_crc = timed(lambda: eng.crc32_device(d_e.data_ptr(), n, d_d.data_ptr(), TOTAL, d_c.data_ptr(), sp))
    k = min(n, 512)
    want = np.array([zlib.crc32(host[i * size:(i + 1) * size].tobytes()) for i in range(k)], dtype=np.uint32)
    assert np.array_equal(d_c[:k].cpu().numpy().view(np.uint32), want), label
    # segment build (segments of at most 4096 entries / 64 MB are the reference's; one image of n entries times the
    # same kernel on the same bytes, max_count capped at the format's 65535)
    nb = min(n, 65535)
    offs_out, size_out = engine.segment_layout(ents[:nb], nb)
    d_f = torch.from_numpy(offs_out.view(np.uint8)).cuda()
    d_o = torch.zeros(size_out, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    us_build = timed(lambda: eng.segment_build_device(d_e.data_ptr(), nb, nb, d_f.data_ptr(), d_d.data_ptr(), TOTAL,
                                                      d_o.data_ptr(), size_out, 0, sp))
    img = d_o[:8 + 32 * 4].cpu().numpy().tobytes()
    import struct
    assert img[:8] == struct.pack(">4sHH", b"RASG", 2, nb) and struct.unpack(">I", img[8 + 28:8 + 32])[0] == int(want[0]), label
    build_payload = int(lens[:nb].sum())
    # (b) the WAL kernels on the same payloads
    went = np.zeros(n, dtype=abi.WAL_ENTRY_DTYPE)
    for f in ("index", "term", "data_offset", "data_len"):
        went[f] = ents[f]
    d_we = torch.from_numpy(went.view(np.uint8)).cuda()
    us_adler = timed(lambda: eng.wal_adler32_device(d_we.data_ptr(), n, d_d.data_ptr(), TOTAL + 16, d_c.data_ptr(), sp))
    recs = np.zeros(nb, dtype=abi.WAL_RECORD_DTYPE)
    for f in ("index", "term", "data_offset", "data_len"):
        recs[f] = ents[f][:nb]
    recs["hdr_offset"] = 0; recs["hdr_len"] = 3
    fr_bytes = engine.wal_layout(recs, 0)
    d_r = torch.from_numpy(recs.view(np.uint8)).cuda()
    d_fo = torch.zeros(fr_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    us_frame = timed(lambda: eng.wal_frame_device(d_r.data_ptr(), nb, d_d.data_ptr(), TOTAL + 16, d_fo.data_ptr(),
                                                  fr_bytes, 0, 0, sp))
    # (a) zlib on the host
    s1, s16 = host_zlib(host, offs, lens, 1), host_zlib(host, offs, lens, 16)
    gb = TOTAL / 1e9
    row = {"workload": label, "entries": n, "payload_bytes": TOTAL,
           "crc32_device_us": us_crc, "crc32_device_GBps": gb / (us_crc * 1e-6),
           "segment_build_entries": nb, "segment_build_us": us_build,
           "segment_build_payload_GBps": build_payload / 1e9 / (us_build * 1e-6),
           "wal_adler32_device_GBps": gb / (us_adler * 1e-6),
           "wal_frame_device_payload_GBps": build_payload / 1e9 / (us_frame * 1e-6),
           "zlib_crc32_1_thread_GBps": gb / s1, "zlib_crc32_16_threads_GBps": gb / s16}
    row["crc32_vs_zlib16"] = row["crc32_device_GBps"] / row["zlib_crc32_16_threads_GBps"]
    row["build_vs_zlib16"] = row["segment_build_payload_GBps"] / row["zlib_crc32_16_threads_GBps"]
    row["crc32_vs_adler32"] = row["crc32_device_GBps"] / row["wal_adler32_device_GBps"]
    row["build_vs_frame"] = row["segment_build_payload_GBps"] / row["wal_frame_device_payload_GBps"]
    res.append(row)
    print(json.dumps(row), flush=True)
    del d_d, d_e, d_c, d_o, d_f, d_we, d_r, d_fo

# one 64 MiB stream
N = 64 << 20
d_d = torch.randint(0, 256, (N,), dtype=torch.uint8, device="cuda")
host = d_d.cpu().numpy()
d_c = torch.zeros(1, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
us = timed(lambda: eng.crc32_stream_device(d_d.data_ptr(), N, 0, d_c.data_ptr(), sp))
assert int(d_c.cpu().numpy().view(np.uint32)[0]) == zlib.crc32(host.tobytes())
t0 = time.perf_counter(); zlib.crc32(memoryview(host)); s1 = time.perf_counter() - t0
# 16 threads on one buffer: sixteen pieces, combined as the kernel combines them -- the pieces alone are timed
s16 = host_zlib(host, np.arange(16, dtype=np.uint64) * (N // 16), np.full(16, N // 16), 16)
row = {"workload": "one 64 MiB stream", "payload_bytes": N, "crc32_stream_device_us": us,
       "crc32_stream_device_GBps": N / 1e9 / (us * 1e-6), "zlib_crc32_1_thread_GBps": N / 1e9 / s1,
       "zlib_crc32_16_threads_GBps": N / 1e9 / s16}
row["stream_vs_zlib16"] = row["crc32_stream_device_GBps"] / row["zlib_crc32_16_threads_GBps"]
res.append(row)
print(json.dumps(row), flush=True)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "segment_bench.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
eng.close()
