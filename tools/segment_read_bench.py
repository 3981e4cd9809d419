#!/usr/bin/env python3
"""One batched read (include/ra_gpu_wal.h: rgb_segment_read_device) against the only device route to the same bytes
that existed before it: one rgb_segment_compact_device call per source, with the wanted indexes as that source's live
list (it builds a segment image per source that nobody asked for, in index order).  Shapes: 65 536 sources x 4 entries
x 256 B and 4 096 x 64 x 4 KiB, each as monotone full-range folds (every index, ascending) and as shuffled sparse
requests (a quarter of the indexes, shuffled), and the larger one once more over files with a backwards step, whose
lookups go through the table of effective records.  Both ways with and without VERIFY.  Device-resident forms, HIP
events around the calls after a warm-up, five repeats.  Beside them: bytes/s of ONE rgb_segment_build_device image of
4096 entries with the same payload bytes, the unit's copy-plus-CRC ceiling.  Every timed output is checked: the rows,
results, total and `out` of the read against the payloads the host packed, the per-source images against the same.
Writes its rows as JSON to profiles/segment_read_bench.json (or argv[1])."""
import json, os, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

REC = np.dtype([("idx", ">u8"), ("term", ">u8"), ("off", ">u8"), ("len", ">u4"), ("crc", ">u4")])
WARM, REPEATS, READ_REPS = 2, 5, 20
SHAPES = [  # name, sources, records per source, payload bytes, requests per source, shuffled, backwards step
    ("fold_65536x4x256", 65536, 4, 256, 4, False, False),
    ("sparse_65536x4x256", 65536, 4, 256, 1, True, False),
    ("fold_4096x64x4096", 4096, 64, 4096, 64, False, False),
    ("sparse_4096x64x4096", 4096, 64, 4096, 16, True, False),
    ("sparse_trimmed_4096x64x4096", 4096, 64, 4096, 16, True, True),
]


def make_case(n_src, per, size, k, shuffled, trimmed, payloads, rng):
    """payloads: uint8[n_src, per, size].  -> (files uint8[n_src, file_len], record number of every request
    int64[n_src, k], requests uint64[n_src * k], Idx of every record int64[per]).  Monotone: record j has Idx j + 1.
    trimmed: the last quarter of the records repeats the Idx of the quarter in front of it (a backwards step): those
    earlier records are trimmed, per * 3 / 4 keys remain."""
    idx_of = np.arange(1, per + 1)
    if trimmed:
        q = per // 4
        idx_of[per - q:] = idx_of[per - 2 * q:per - q]
    keys = np.unique(idx_of)
    rec_of_key = {int(i): int(np.flatnonzero(idx_of == i)[-1]) for i in keys}        # the later record wins
    data_start = 8 + 32 * per
    files = np.zeros((n_src, data_start + per * size), dtype=np.uint8)
    files[:, :8] = np.frombuffer(b"RASG" + bytes([0, 2, per >> 8, per & 0xFF]), dtype=np.uint8)
    recs = np.zeros((n_src, per), dtype=REC)
    recs["idx"], recs["term"] = idx_of, 3
    recs["off"], recs["len"] = data_start + np.arange(per) * size, size
    recs["crc"] = np.array([zlib.crc32(p) for p in payloads.reshape(-1, size)], dtype=np.uint32).reshape(n_src, per)
    files[:, 8:data_start] = recs.view(np.uint8).reshape(n_src, 32 * per)
    files[:, data_start:] = payloads.reshape(n_src, per * size)
    if shuffled:
        asked = np.stack([rng.permutation(keys)[:k] for _ in range(n_src)])
    else:
        asked = np.tile(keys[:k], (n_src, 1))
    rec_no = np.vectorize(rec_of_key.get)(asked)
    return files, rec_no, asked.astype(np.uint64).reshape(-1), idx_of


def ranges_of(indexes):
    out = []
    for i in sorted(int(x) for x in indexes):
        if out and i == out[-1][1] + 1:
            out[-1][1] = i
        else:
            out.append([i, i])
    return out


def main():
    import torch
    from ra_amd import abi, engine
    assert torch.cuda.is_available(), "segment_read_bench.py measures on the GPU; there is no CPU fallback"
    eng = engine.RaGpuBatch(1, 1)
    stream = torch.cuda.Stream(); sp = stream.cuda_stream

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
    rng = np.random.default_rng(41)
    for name, n_src, per, size, k, shuffled, trimmed in SHAPES:
        payloads = torch.randint(0, 256, (n_src, per, size), dtype=torch.uint8, device="cuda").cpu().numpy()
        files, rec_no, req, idx_of = make_case(n_src, per, size, k, shuffled, trimmed, payloads, rng)
        file_len, n_req, total = files.shape[1], n_src * k, n_src * k * size
        row = {"shape": name, "sources": n_src, "records_per_source": per, "payload_bytes": size, "requests_per_source": k,
               "requests": n_req, "total_payload_bytes": total, "files_bytes": int(files.size), "repeats": REPEATS,
               "request_order": "shuffled" if shuffled else "ascending", "backwards_step": trimmed}
        want_out = payloads[np.arange(n_src)[:, None], rec_no].reshape(-1)
        sources = np.zeros(n_src, dtype=abi.SEG_READ_SOURCE_DTYPE)
        sources["offset"], sources["n_bytes"] = np.arange(n_src, dtype=np.uint64) * file_len, file_len
        sources["req_first"], sources["req_n"] = np.arange(n_src) * k, k
        d_files = torch.from_numpy(files.reshape(-1)).cuda()
        d_rows = torch.zeros(32 * n_req, dtype=torch.uint8, device="cuda")
        d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros(32 * n_src, dtype=torch.uint8, device="cuda")
        d_tot = torch.zeros(16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        times = {}
        for flags, tag in ((0, "read_one_call"), (abi.SEG_READ_VERIFY, "read_one_call_verify")):
            def read():
                eng.segment_read_device(sources, d_files.data_ptr(), files.size, req, d_rows.data_ptr(), d_out.data_ptr(),
                                        total, d_res.data_ptr(), d_tot.data_ptr(), flags, sp)
            d_out.zero_(); torch.cuda.synchronize()
            times[tag] = timed(read, READ_REPS, WARM)
            tot = d_tot.cpu().numpy().view(abi.SEG_READ_TOTAL_DTYPE)[0]
            assert (int(tot["status"]), int(tot["n_bad"]), int(tot["out_bytes"])) == (0, 0, total), tot
            results = d_res.cpu().numpy().view(abi.SEG_READ_RESULT_DTYPE)
            assert np.all(results["status"] == 0) and np.all(results["n_read"] == k) and np.all(results["data_bytes"] == k * size)
            rows = d_rows.cpu().numpy().view(abi.SEG_ENTRY_DTYPE)
            assert np.array_equal(rows["index"], req) and np.all(rows["term"] == 3) and np.all(rows["data_len"] == size)
            assert np.array_equal(rows["data_offset"], np.arange(n_req, dtype=np.uint64) * size)
            assert np.array_equal(d_out.cpu().numpy(), want_out), f"{name}: the bytes of the read differ"

        # the parent's route: one rgb_segment_compact_device call per source, the wanted indexes as its live list
        lives = [ranges_of(req[s * k:(s + 1) * k]) for s in range(n_src)]
        image = 8 + 32 * k + file_len                       # rgb_segment_compact_bound of one source
        d_img = torch.zeros(n_src * image, dtype=torch.uint8, device="cuda")
        d_cres = torch.zeros(32 * n_src, dtype=torch.uint8, device="cuda")
        one = [(sources[s:s + 1].view(abi.SEG_SOURCE_DTYPE).copy(), np.array(lives[s], dtype=np.uint64).reshape(-1, 2))
               for s in range(n_src)]
        for s in range(n_src):
            one[s][0]["offset"], one[s][0]["live_first"], one[s][0]["live_n"] = 0, 0, len(lives[s])
        torch.cuda.synchronize()
        p_f, p_img, p_r = d_files.data_ptr(), d_img.data_ptr(), d_cres.data_ptr()
        for flags, tag in ((0, "compact_per_source"), (abi.SEG_COMPACT_VERIFY, "compact_per_source_verify")):
            def per_source():
                for s in range(n_src):
                    eng.segment_compact_device(one[s][0], p_f + file_len * s, file_len, one[s][1], p_img + image * s, image,
                                               p_r + 32 * s, abi.SEG_MAX_SIZE_B, flags, sp)
            times[tag] = timed(per_source, 1, 1)
            cres = d_cres.cpu().numpy().view(abi.SEG_COMPACT_RESULT_DTYPE)
            assert np.all(cres["status"] == 0) and np.all(cres["n_entries"] == k), f"{name}: a per-source compaction failed"
            imgs = d_img.cpu().numpy().reshape(n_src, image)[:, 8 + 32 * k:8 + 32 * k + k * size]
            order = np.argsort(req.reshape(n_src, k), axis=1)                    # the image holds them in index order
            want_img = payloads[np.arange(n_src)[:, None], np.take_along_axis(rec_no, order, axis=1)].reshape(n_src, k * size)
            assert np.array_equal(imgs, want_img), f"{name}: the per-source images differ"
        del d_img, d_cres, one, imgs

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
        times["build_one_image"] = timed(lambda: eng.segment_build_device(d_be.data_ptr(), big_n, big_n, d_bf.data_ptr(),
                                                                          d_out.data_ptr(), total, d_b.data_ptr(), big_size, 0, sp),
                                         READ_REPS, WARM)
        assert np.array_equal(d_b.cpu().numpy()[8 + 32 * big_n:], want_out[:big_n * big_len]), f"{name}: the one image differs"
        for tag, (med, lo, hi) in times.items():
            row[tag + "_us"], row[tag + "_us_min"], row[tag + "_us_max"] = med, lo, hi
            row[tag + "_GBps"] = total / 1e9 / (med * 1e-6)
        for v in ("", "_verify"):
            a, b = times["read_one_call" + v], times["compact_per_source" + v]
            row["one_call_vs_per_source" + v] = b[0] / a[0]                      # > 1: the one call is faster
            row["faster_beyond_spread" + v] = bool(a[2] < b[1])                  # its slowest repeat under their fastest
        row["verify_share_of_ceiling"] = times["build_one_image"][0] / times["read_one_call_verify"][0]
        row["plain_share_of_ceiling"] = times["build_one_image"][0] / times["read_one_call"][0]
        res.append(row)
        print(json.dumps(row), flush=True)
        del d_files, d_rows, d_out, d_res, d_tot, d_b, d_be, d_bf, files, payloads, want_out

    res.append({"not_measured": "NO_DATA (term queries), version-1 sources, the host-buffer form (PCIe-inclusive), sources of "
                                "more than 64 records, kernel time by pass (no profiler run), the wavefront-per-row VERIFY copy at 7 "
                                "against 8 wavefronts per SIMD"})
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "segment_read_bench.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    eng.close()


if __name__ == "__main__":
    main()
