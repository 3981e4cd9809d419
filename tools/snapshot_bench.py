#!/usr/bin/env python3
"""The batched snapshot calls (include/ra_gpu_wal.h: rgb_snapshot_build_device, rgb_snapshot_validate_device,
rgb_crc32_spans_device) against the routes the library offered before them for the same bytes, in the same process:
one rgb_crc32_stream_device call per file, one rgb_crc32_device call with an entry per file, and -- as the unit's
copy-plus-CRC ceiling -- rgb_segment_build_device over the same payload bytes as ONE image of 4096 entries.  Shapes (the
Data of each snapshot; every file has 64 bytes of Meta): 65 536 x 1 KiB, 8 x 256 MiB, 16 384 files log-uniform from 64 B
to 1 MiB, and the skewed batch of one 1 GiB file beside 65 536 x 512 B.  Device-resident forms, HIP events around the
calls after a warm-up, five repeats; the descriptor arrays are host arrays, so the time of the batched calls includes
their planning on the host and the upload of the plan.  Every timed output is checked: the images against the bytes the
host packed, every CRC and info row against zlib.  Writes its rows as JSON to profiles/snapshot_bench.json (or argv[1])."""
import json, os, struct, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

WARM, REPEATS, META = 1, 5, 64


def shapes(rng):
    yield "65536x1KiB", np.full(65536, 1024, dtype=np.int64), 10
    yield "8x256MiB", np.full(8, 256 << 20, dtype=np.int64), 3
    yield "16384_loguniform_64B_1MiB", np.exp(rng.uniform(np.log(64), np.log(1 << 20), size=16384)).astype(np.int64), 3
    yield "skewed_1GiB_and_65536x512B", np.concatenate([[1 << 30], np.full(65536, 512)]).astype(np.int64), 3


def main():
    import torch
    from ra_amd import abi, engine
    assert torch.cuda.is_available(), "snapshot_bench.py measures on the GPU; there is no CPU fallback"
    eng = engine.RaGpuBatch(1, 1)
    stream = torch.cuda.Stream(); sp = stream.cuda_stream

    def timed(fn, reps, warm=WARM):
        """us per call of fn: (median, min, max) over REPEATS measurements of `reps` calls"""
        out = []
        for _ in range(REPEATS):
            with torch.cuda.stream(stream):
                for _ in range(warm):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(reps):
                    fn()
                e1.record(stream)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / reps)
        return float(np.median(out)), float(min(out)), float(max(out))

    res = []
    rng = np.random.default_rng(51)
    head_crc = zlib.crc32(struct.pack(">I", META))
    for name, sizes, reps in shapes(rng):
        n = len(sizes)
        src_off = np.concatenate([[0], np.cumsum(sizes + META)[:-1]]).astype(np.uint64)     # Meta, then Data, back to back
        total = int((sizes + META).sum())
        d_data = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
        host = d_data.cpu().numpy()
        want_crc = np.array([zlib.crc32(host[int(o):int(o) + META + int(s)], head_crc) for o, s in zip(src_off, sizes)],
                            dtype=np.uint32)
        items = np.zeros(n, dtype=abi.SNAP_ITEM_DTYPE)
        items["meta_len"], items["meta_offset"] = META, src_off
        items["data_offset"], items["data_bytes"] = src_off + np.uint64(META), sizes
        items, out_size = engine.snapshot_layout(items)
        file_off = items["out_offset"].copy()
        file_len = (sizes + META + 13).astype(np.uint64)
        row = {"shape": name, "files": n, "payload_bytes": total, "largest_file": int(file_len.max()),
               "smallest_file": int(file_len.min()), "repeats": REPEATS}
        d_out = torch.zeros(out_size, dtype=torch.uint8, device="cuda")
        d_crcs = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_rows = torch.zeros(n * abi.SNAP_INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        times = {}

        # writing: every image in one call
        times["build"] = timed(lambda: eng.snapshot_build_device(items, d_data.data_ptr(), total, d_out.data_ptr(), out_size,
                                                                 d_crcs.data_ptr(), sp), reps)
        assert np.array_equal(d_crcs.cpu().numpy().view(np.uint32), want_crc), f"{name}: the CRCs of the images differ"
        out = d_out.cpu().numpy()
        for i in range(n):
            o, s = int(file_off[i]), int(src_off[i])
            assert out[o:o + 13].tobytes() == struct.pack(">4sBII", b"RASN", 1, int(want_crc[i]), META), f"{name}: header {i}"
            assert np.array_equal(out[o + 13:o + int(file_len[i])], host[s:s + META + int(sizes[i])]), f"{name}: image {i}"
        del out

        # recovery: every file validated in one call
        files = np.zeros(n, dtype=abi.SNAP_FILE_DTYPE)
        files["offset"], files["n_bytes"] = file_off, file_len
        times["validate"] = timed(lambda: eng.snapshot_validate_device(files, d_out.data_ptr(), out_size, d_rows.data_ptr(), sp), reps)
        rows = d_rows.cpu().numpy().view(abi.SNAP_INFO_DTYPE)
        assert np.all(rows["status"] == abi.SNAP_OK) and np.array_equal(rows["stored_crc"], want_crc)
        assert np.array_equal(rows["computed_crc"], want_crc) and np.all(rows["meta_len"] == META)
        assert np.array_equal(rows["data_bytes"], sizes.astype(np.uint64)) and \
            np.array_equal(rows["data_offset"], file_off + np.uint64(13 + META))

        # receiving: the same bytes as one ragged batch of spans
        spans = np.zeros(n, dtype=abi.CRC_SPAN_DTYPE)
        spans["offset"], spans["n_bytes"] = file_off + np.uint64(9), file_len - np.uint64(9)
        d_crcs.zero_(); torch.cuda.synchronize()
        times["spans"] = timed(lambda: eng.crc32_spans_device(spans, d_out.data_ptr(), out_size, d_crcs.data_ptr(), sp), reps)
        assert np.array_equal(d_crcs.cpu().numpy().view(np.uint32), want_crc), f"{name}: the CRCs of the spans differ"

        # the parent's routes over the same bytes: a stream call per file ...
        p_out, p_c = d_out.data_ptr(), d_crcs.data_ptr()
        offs, lens = [int(x) + 9 for x in file_off], [int(x) - 9 for x in file_len]
        d_crcs.zero_(); torch.cuda.synchronize()

        def per_file():
            for i in range(n):
                eng.crc32_stream_device(p_out + offs[i], lens[i], 0, p_c + 4 * i, sp)
        times["stream_per_file"] = timed(per_file, 1)
        assert np.array_equal(d_crcs.cpu().numpy().view(np.uint32), want_crc), f"{name}: the per-file stream CRCs differ"
        # ... and one per-entry call (a file is one entry: at most a wavefront, a 32-bit length)
        entries = np.zeros(n, dtype=abi.SEG_ENTRY_DTYPE)
        entries["data_offset"], entries["data_len"] = spans["offset"], spans["n_bytes"]
        d_e = torch.from_numpy(entries.view(np.uint8)).cuda()
        d_crcs.zero_(); torch.cuda.synchronize()
        times["crc32_entry_per_file"] = timed(lambda: eng.crc32_device(d_e.data_ptr(), n, p_out, out_size, p_c, sp), reps)
        assert np.array_equal(d_crcs.cpu().numpy().view(np.uint32), want_crc), f"{name}: the per-entry CRCs differ"

        # the ceiling: one segment image of 4096 entries over the same payload bytes
        big_n, big_len = 4096, total // 4096
        big = np.zeros(big_n, dtype=abi.SEG_ENTRY_DTYPE)
        big["index"] = 1 + np.arange(big_n); big["term"] = 3; big["data_len"] = big_len
        big["data_offset"] = np.arange(big_n, dtype=np.uint64) * np.uint64(big_len)
        big_offs, big_size = engine.segment_layout(big, big_n)
        d_be = torch.from_numpy(big.view(np.uint8)).cuda()
        d_bf = torch.from_numpy(big_offs.view(np.uint8)).cuda()
        d_b = torch.zeros(big_size, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        times["segment_build_ceiling"] = timed(lambda: eng.segment_build_device(d_be.data_ptr(), big_n, big_n, d_bf.data_ptr(),
                                                                                d_data.data_ptr(), total, d_b.data_ptr(), big_size,
                                                                                0, sp), reps)
        assert np.array_equal(d_b.cpu().numpy()[8 + 32 * big_n:], host[:big_n * big_len]), f"{name}: the one image differs"

        for tag, (med, lo, hi) in times.items():
            row[tag + "_us"], row[tag + "_us_min"], row[tag + "_us_max"] = med, lo, hi
            row[tag + "_GBps"] = total / 1e9 / (med * 1e-6)
        parents = [times["stream_per_file"], times["crc32_entry_per_file"]]
        best = min(parents, key=lambda t: t[0])
        row["better_parent_route"] = "stream_per_file" if best is parents[0] else "crc32_entry_per_file"
        for tag in ("validate", "spans"):
            ours = times[tag]
            row[tag + "_vs_better_parent"] = best[0] / ours[0]                               # > 1: the batched call is faster
            row[tag + "_not_slower_beyond_spread"] = bool(ours[1] <= best[2])                # its fastest repeat within theirs
            row[tag + "_beats_both_beyond_spread"] = bool(all(ours[2] < p[1] for p in parents))
        row["build_share_of_ceiling"] = times["segment_build_ceiling"][0] / times["build"][0]
        res.append(row)
        print(json.dumps(row), flush=True)
        del d_data, d_out, d_crcs, d_rows, d_e, d_be, d_bf, d_b, host

    res.append({"not_measured": "the host-buffer forms (PCIe-inclusive), the indexes kind, META_ONLY batches, the share of "
                                "host planning and plan upload in the batched calls' time, kernel time by pass (no profiler run)"})
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "snapshot_bench.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    eng.close()


if __name__ == "__main__":
    main()
