#!/usr/bin/env python3
"""Many compaction groups: one rgb_segment_compact_groups_device call (B) against a loop of rgb_segment_compact_device,
one call per group (A) -- include/ra_gpu_wal.h, "major compaction for many members in one call".  Both paths run in this
process on the same device-resident files, into the same output layout; HIP events around as many rounds as fill a
window of WINDOW_US (at least MIN_REPS, from a pilot measurement of each path) after WARM warm-up rounds, REPEATS
measurements each, A and B alternating so that neither owns a clock state.  A round of A is
one call per group, a round of B is one call.  Before anything is timed the B images are compared with the A images.

Workloads: 512 groups x 2 sources x 64 live entries of 256 B out of 256 records each -- the many-small-groups case;
the same with 4 KiB payloads; and ONE group equal to the default workload of tools/segment_compact_bench.py (4 sources
of 4096 entries of 256 B, a quarter live) to see what the general path costs a single big group.
Writes its rows as JSON to profiles/segment_compact_groups_bench.json (or argv[1]); argv[2]: only the workload of that
number (for a kernel trace of one workload in a run of its own)."""
import json, os, struct, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from ra_amd import abi, engine

assert torch.cuda.is_available(), "segment_compact_groups_bench.py measures on the GPU; there is no CPU fallback"
eng = engine.RaGpuBatch(1, 1)
stream = torch.cuda.Stream(); sp = stream.cuda_stream
MIN_REPS, WARM, REPEATS, WINDOW_US = 5, 2, 7, 1_000_000.0       # a second per window
MAX_SIZE = abi.SEG_MAX_SIZE_B * 8
REC = np.dtype([("idx", ">u8"), ("term", ">u8"), ("off", ">u8"), ("len", ">u4"), ("crc", ">u4")])


def once(fn, reps):
    """us per round: one measurement of `reps` rounds"""
    with torch.cuda.stream(stream):
        for _ in range(WARM):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def workload(n_groups, per_group, records, size, live_of_16):
    """n_groups groups of per_group sources of `records` records of `size` bytes; of every sixteen records the first
    live_of_16 are live.  The payload bytes are random, the stored Crc 0 ("not checked"): the copy is what is timed."""
    data_start = 8 + 32 * records
    file_bytes = data_start + records * size
    n_sources = n_groups * per_group
    total = n_sources * file_bytes
    d_files = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
    files_view = d_files.view(n_sources, file_bytes)
    sources = np.zeros(n_sources, dtype=abi.SEG_SOURCE_DTYPE)
    live = np.zeros((n_sources * (records // 16), 2), dtype=np.uint64)
    for s in range(n_sources):
        first = 1 + s * records
        index = np.zeros(records, dtype=REC)
        index["idx"] = np.arange(first, first + records); index["term"] = 7
        index["off"] = data_start + np.arange(records, dtype=np.uint64) * size
        index["len"] = size
        head = np.frombuffer(struct.pack(">4sHH", b"RASG", 2, records) + index.tobytes(), dtype=np.uint8)
        files_view[s, :data_start] = torch.from_numpy(head.copy()).cuda()
        sources["offset"][s], sources["n_bytes"][s] = s * file_bytes, file_bytes
        sources["live_first"][s], sources["live_n"][s] = s * (records // 16), records // 16
        k = np.arange(records // 16, dtype=np.uint64)
        live[s * (records // 16):(s + 1) * (records // 16), 0] = first + 16 * k
        live[s * (records // 16):(s + 1) * (records // 16), 1] = first + 16 * k + live_of_16 - 1
    groups = np.zeros(n_groups, dtype=abi.SEG_GROUP_DTYPE)
    groups["src_first"], groups["src_n"] = np.arange(n_groups) * per_group, per_group
    live_per_group = per_group * (records // 16) * live_of_16
    image = 8 + 32 * live_per_group + live_per_group * size
    groups["out_offset"], groups["out_bytes"] = np.arange(n_groups, dtype=np.uint64) * image, image
    return d_files, total, sources, live, groups, image, live_per_group


res = []
ONLY = int(sys.argv[2]) if len(sys.argv) > 2 else None
for number, (label, shape) in enumerate((("512 groups x 2 sources x 64 live of 256 records, 256 B", (512, 2, 256, 256, 4)),
                     ("512 groups x 2 sources x 64 live of 256 records, 4 KiB", (512, 2, 256, 4096, 4)),
                     ("1 group x 4 sources x 1024 live of 4096 records, 256 B", (1, 4, 4096, 256, 4)))):
    if ONLY is not None and number != ONLY:
        continue
    n_groups = shape[0]
    d_files, total, sources, live, groups, image, live_per_group = workload(*shape)
    out_bytes = n_groups * image
    d_a = torch.zeros(out_bytes, dtype=torch.uint8, device="cuda")
    d_b = torch.zeros(out_bytes, dtype=torch.uint8, device="cuda")
    d_ra = torch.zeros(32 * n_groups, dtype=torch.uint8, device="cuda")
    d_rb = torch.zeros(32 * n_groups, dtype=torch.uint8, device="cuda")
    per = [sources[int(g["src_first"]):int(g["src_first"]) + int(g["src_n"])].copy() for g in groups]
    torch.cuda.synchronize()

    def path_a(flags=0):
        for g in range(n_groups):
            eng.segment_compact_device(per[g], d_files.data_ptr(), total, live, d_a.data_ptr() + g * image, image,
                                       d_ra.data_ptr() + 32 * g, MAX_SIZE, flags, sp)

    def path_b(flags=0):
        eng.segment_compact_groups_device(groups, sources, d_files.data_ptr(), total, live, d_b.data_ptr(), out_bytes,
                                          d_rb.data_ptr(), MAX_SIZE, flags, sp)
    path_a(); path_b()
    eng.synchronize(); torch.cuda.synchronize()
    ra = d_ra.cpu().numpy().view(abi.SEG_COMPACT_RESULT_DTYPE)
    rb = d_rb.cpu().numpy().view(abi.SEG_COMPACT_RESULT_DTYPE)
    assert np.all(ra["status"] == 0) and np.all(ra["n_entries"] == live_per_group) and np.all(ra["file_bytes"] == image), label
    assert ra.tobytes() == rb.tobytes(), f"{label}: the result rows differ"
    assert torch.equal(d_a, d_b), f"{label}: the images of the batched call differ from the calls per group"
    reps_a = max(MIN_REPS, min(20000, int(WINDOW_US / once(path_a, MIN_REPS)) + 1))
    reps_b = max(MIN_REPS, min(20000, int(WINDOW_US / once(path_b, MIN_REPS)) + 1))
    a, b = [], []
    for _ in range(REPEATS):
        a.append(once(path_a, reps_a))
        b.append(once(path_b, reps_b))
    row = {"workload": label, "groups": n_groups, "sources": len(sources), "live_entries": int(n_groups * live_per_group),
           "live_payload_bytes": int(n_groups * live_per_group * shape[3]), "source_bytes": int(total),
           "repeats": REPEATS, "A_rounds_per_repeat": reps_a, "B_rounds_per_repeat": reps_b,
           "A_calls_per_group_us": float(np.median(a)), "A_us_min": float(min(a)), "A_us_max": float(max(a)),
           "A_spread": float((max(a) - min(a)) / np.median(a)),
           "B_one_call_us": float(np.median(b)), "B_us_min": float(min(b)), "B_us_max": float(max(b)),
           "A_over_B": float(np.median(a) / np.median(b))}
    res.append(row)
    print(json.dumps(row), flush=True)
    del d_files, d_a, d_b, d_ra, d_rb

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "segment_compact_groups_bench.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
eng.close()
