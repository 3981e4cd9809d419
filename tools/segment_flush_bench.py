#!/usr/bin/env python3
"""One batched mem-table flush (include/ra_gpu_wal.h: rgb_segment_flush_device) against the way the same work was done
before it existed: W calls of rgb_segment_build_device, one per writer, over the same entries.  W in {4 096, 65 536}
writers, 4 and 32 entries per writer, 256 B and 4 KiB payloads (a combination whose payloads exceed 2 GiB is listed as
not measured).  Device-resident forms, HIP events around the calls after a warm-up, five repeats; the writers' open
segments are fresh (MaxCount 64), the per-writer images of the old way have MaxCount = entries per writer, the
smallest image there is.  Beside both: bytes/s of ONE rgb_segment_build_device image of the same payload bytes (4096
entries), the ceiling of a CRC-and-copy pass.  Every timed output is checked: the flush by applying its pieces and
comparing every file with the sequential referee of tests/test_segment_flush.py, the images with
tests/test_segment.py::python_segment.  Writes its rows as JSON to profiles/segment_flush_bench.json (or argv[1])."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from ra_amd import abi, engine

assert torch.cuda.is_available(), "segment_flush_bench.py measures on the GPU; there is no CPU fallback"
from test_segment import python_segment
from test_segment_flush import RefFile, UNDEF, check_answer

eng = engine.RaGpuBatch(1, 1)
stream = torch.cuda.Stream(); sp = stream.cuda_stream
WARM, REPEATS, FLUSH_REPS = 2, 5, 20
OPEN_MAX, MAX_BYTES = 64, 2 << 30


def timed(fn, reps, warm):
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
for n_w in (4096, 65536):
    for per in (4, 32):
        for size in (256, 4096):
            n, total = n_w * per, n_w * per * size
            row = {"writers": n_w, "entries_per_writer": per, "payload_bytes": size, "entries": n, "total_payload_bytes": total,
                   "repeats": REPEATS}
            if total > MAX_BYTES:
                row["not_measured"] = f"{total} payload bytes exceed the {MAX_BYTES} of this tool"
                res.append(row); print(json.dumps(row), flush=True)
                continue
            d_data = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
            host = d_data.cpu().numpy()
            entries = np.zeros(n, dtype=abi.SEG_ENTRY_DTYPE)
            entries["index"] = 1 + np.arange(n) % per; entries["term"] = 3
            entries["data_offset"] = np.arange(n, dtype=np.uint64) * size; entries["data_len"] = size
            writers = np.zeros(n_w, dtype=abi.SEG_WRITER_DTYPE)
            writers["entry_first"] = np.arange(n_w) * per; writers["entry_n"] = per
            writers["open_max_count"] = OPEN_MAX; writers["range_first"] = writers["range_last"] = UNDEF
            out_bound, pieces_bound = engine.segment_flush_bound(writers, n, total)
            d_e = torch.from_numpy(entries.view(np.uint8)).cuda()
            d_out = torch.zeros(out_bound, dtype=torch.uint8, device="cuda")
            d_p = torch.zeros(80 * pieces_bound, dtype=torch.uint8, device="cuda")
            d_r = torch.zeros(32, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def flush():
                eng.segment_flush_device(writers, d_e.data_ptr(), n, d_data.data_ptr(), total, d_p.data_ptr(), pieces_bound,
                                         d_out.data_ptr(), out_bound, d_r.data_ptr(), OPEN_MAX, abi.SEG_MAX_SIZE_B, 0, sp)
            t_flush = timed(flush, FLUSH_REPS, WARM)
            r = d_r.cpu().numpy().view(abi.SEG_FLUSH_RESULT_DTYPE)[0]
            assert (int(r["status"]), int(r["n_pieces"]), int(r["out_bytes"])) == (0, n_w, total + 32 * n), r
            pieces = d_p.cpu().numpy()[:80 * n_w].view(abi.SEG_PIECE_DTYPE)
            out = d_out.cpu().numpy()[:int(r["out_bytes"])]
            empty = python_segment([], [], OPEN_MAX)
            payloads = [host[j * size:(j + 1) * size].tobytes() for j in range(n)]
            specs = [dict(open=RefFile(OPEN_MAX, empty), entries=[(1 + k, 3, payloads[w * per + k]) for k in range(per)])
                     for w in range(n_w)]
            batches = [[(w * per + k, 1 + k, 3, payloads[w * per + k]) for k in range(per)] for w in range(n_w)]
            check_answer(specs, batches, OPEN_MAX, abi.SEG_MAX_SIZE_B, 0, r, pieces, out.tobytes(), json.dumps(row))
            del specs, batches, out, pieces

            # the old way: one rgb_segment_build_device call per writer, MaxCount = entries per writer
            image = 8 + 32 * per + per * size
            offs = np.tile(8 + 32 * per + np.arange(per, dtype=np.uint64) * size, n_w)
            local = entries.copy(); local["data_offset"] = np.tile(np.arange(per, dtype=np.uint64) * size, n_w)
            d_le = torch.from_numpy(local.view(np.uint8)).cuda()
            d_f = torch.from_numpy(offs.view(np.uint8)).cuda()
            d_img = torch.zeros(n_w * image, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            p_le, p_f, p_d, p_img = d_le.data_ptr(), d_f.data_ptr(), d_data.data_ptr(), d_img.data_ptr()

            def per_writer():
                for w in range(n_w):
                    eng.segment_build_device(p_le + 32 * per * w, per, per, p_f + 8 * per * w, p_d + per * size * w, per * size,
                                             p_img + image * w, image, 0, sp)
            t_calls = timed(per_writer, 1, 1)
            imgs = d_img.cpu().numpy()
            for w in range(n_w):
                want = python_segment([(1 + k, 3) for k in range(per)], payloads[w * per:(w + 1) * per], per)
                assert imgs[w * image:(w + 1) * image].tobytes() == want, f"writer {w}: the per-writer image differs"
            del imgs, d_img, d_le, d_f

            # the ceiling: one image of 4096 entries with the same payload bytes
            big_n, big_len = 4096, total // 4096
            big = np.zeros(big_n, dtype=abi.SEG_ENTRY_DTYPE)
            big["index"] = 1 + np.arange(big_n); big["term"] = 3; big["data_len"] = big_len
            big["data_offset"] = np.arange(big_n, dtype=np.uint64) * big_len
            big_offs, big_size = engine.segment_layout(big, big_n)
            d_be = torch.from_numpy(big.view(np.uint8)).cuda()
            d_bf = torch.from_numpy(big_offs.view(np.uint8)).cuda()
            d_b = torch.zeros(big_size, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            t_big = timed(lambda: eng.segment_build_device(d_be.data_ptr(), big_n, big_n, d_bf.data_ptr(), d_data.data_ptr(), total,
                                                           d_b.data_ptr(), big_size, 0, sp), FLUSH_REPS, WARM)
            got = d_b.cpu().numpy()
            assert got.tobytes() == python_segment([(1 + j, 3) for j in range(big_n)],
                                                   [host[j * big_len:(j + 1) * big_len].tobytes() for j in range(big_n)], big_n)
            for name, (med, lo, hi) in (("flush_one_call", t_flush), ("build_per_writer", t_calls), ("build_one_image", t_big)):
                row[name + "_us"], row[name + "_us_min"], row[name + "_us_max"] = med, lo, hi
                row[name + "_GBps"] = total / 1e9 / (med * 1e-6)
            row["one_call_vs_per_writer"] = t_calls[0] / t_flush[0]                    # > 1: the one call is faster
            row["faster_beyond_spread"] = bool(t_flush[2] < t_calls[1])                # its slowest repeat under their fastest
            row["one_call_share_of_ceiling"] = t_big[0] / t_flush[0]
            res.append(row)
            print(json.dumps(row), flush=True)
            del d_data, d_out, d_p, d_e, d_b, d_be, d_bf, host, payloads, got

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "segment_flush_bench.json")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
eng.close()
