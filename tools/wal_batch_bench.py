#!/usr/bin/env python3
"""One rgb_wal_batch_device call (include/ra_gpu_wal.h, "WAL batch") against the way the same batch was served before it
existed: the per-record loop of ra_log_wal:handle_batch/2 on the host -- verdicts, serialize_header/3, the roll test, the
batch writers' sequences; host C++ compiled by this tool, HOST_LOOP below -- then rgb_wal_layout, the upload of records
and header bytes, and one rgb_wal_frame_device call.

  (a) 64 Ki commands of 16 Ki writers, 256-byte and 4 KiB payloads
  (c) 64 Ki commands of ONE writer, 256-byte payloads: what the serial chain costs
  (b) the frame kernels alone are not separable with HIP events: run this tool with --kernels-only under a kernel trace
      (tools: rocprofv3 --kernel-trace --stats) and compare rgb_wal_batch_frame_kernel with rgb_wal_frame_kernel there.

Device-resident payloads, HIP events around the calls after a warm-up (the events bracket the host work of a call too:
the stream is idle while the host loops), five repeats.  Every timed output is checked: the framed bytes of both ways
are equal; rows, writers, bytes and events of (a) against the referee of tests/test_wal_batch.py, those of (c) against
the host loop (the referee's ra_seq restatement is quadratic in a writer's commands).  Writes its rows as JSON to
profiles/wal_batch_bench.json (or argv[1])."""
import ctypes, hashlib, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from ra_amd import abi, engine

assert torch.cuda.is_available(), "wal_batch_bench.py measures on the GPU; there is no CPU fallback"

HOST_LOOP = r"""
#include <stdint.h>
#include <string.h>
#include <vector>
#include "ra_gpu_wal.h"
struct run { uint64_t term, tid, floor; std::vector<uint64_t> pairs; };
/* handle_msg/2, write_data/8 without the checksum and the copy, incr_batch/8, complete_batch_writer/3.  -> records
 * written; hdr receives the HeaderData bytes back to back (hdr_offset relative to hdr_base) */
extern "C" uint32_t host_loop(const rgb_wal_cmd *cmds, uint32_t n, rgb_wal_writer *writers, uint32_t n_writers,
                              const unsigned char *uids, rgb_wal_file *file, rgb_wal_record *recs, unsigned char *hdr,
                              uint64_t hdr_base, uint32_t *verdicts, uint64_t *pairs_out, uint32_t *n_pairs,
                              uint32_t *n_events, uint32_t *n_consumed) {
  std::vector<std::vector<run>> waiting(n_writers);
  uint32_t nw = 0;
  uint64_t hp = 0;
  *n_consumed = n;
  for (uint32_t i = 0; i < n; ++i) {
    const rgb_wal_cmd &c = cmds[i];
    rgb_wal_writer &w = writers[c.writer];
    bool trunc = c.index == c.smallest_index;
    if (c.index < c.smallest_index) { w.state = RGB_WAL_W_IN_SEQ; w.prev_index = c.smallest_index - 1; verdicts[i] = RGB_WAL_V_DROP; continue; }
    if (w.state != RGB_WAL_W_UNDEFINED && (c.prev_index <= w.prev_index || trunc)) {}
    else if (w.state == RGB_WAL_W_UNDEFINED) trunc = false;
    else if (w.state == RGB_WAL_W_OUT_OF_SEQ) { verdicts[i] = RGB_WAL_V_IGNORE; continue; }
    else { verdicts[i] = RGB_WAL_V_RESEND; w.state = RGB_WAL_W_OUT_OF_SEQ; continue; }
    if (file->file_size > file->max_size || (file->max_entries && file->entry_count + 1 > file->max_entries)) { *n_consumed = i; break; }
    rgb_wal_record &r = recs[nw++];
    r.index = c.index; r.term = c.term; r.data_offset = c.data_offset; r.data_len = c.data_len; r.hdr_offset = hdr_base + hp;
    uint32_t header_len;
    if (w.id_ref != RGB_WAL_NO_ID_REF) {
      const uint32_t h = (trunc ? 1u << 23 : 0u) | 1u << 22 | w.id_ref;
      hdr[hp] = h >> 16; hdr[hp + 1] = h >> 8; hdr[hp + 2] = h;
      r.hdr_len = 3; header_len = trunc ? 2 : 3;
    } else {
      w.id_ref = file->next_id_ref++;
      const uint32_t h = (trunc ? 1u << 23 : 0u) | w.id_ref;
      hdr[hp] = h >> 16; hdr[hp + 1] = h >> 8; hdr[hp + 2] = h; hdr[hp + 3] = w.uid_len >> 8; hdr[hp + 4] = w.uid_len;
      memcpy(hdr + hp + 5, uids + w.uid_offset, w.uid_len);
      r.hdr_len = header_len = 5 + w.uid_len;
    }
    hp += r.hdr_len;
    verdicts[i] = RGB_WAL_V_WRITE | (trunc ? RGB_WAL_V_TRUNC : 0u);
    std::vector<run> &chain = waiting[c.writer];
    if (chain.empty() || chain.back().term != c.term || chain.back().tid != c.tid) chain.push_back(run{c.term, c.tid, 0, {}});
    run &b = chain.back();
    std::vector<uint64_t> &p = b.pairs;                   /* (first, last) pairs: limit(Idx - 1), then append */
    while (!p.empty() && p[p.size() - 2] >= c.index) { p.pop_back(); p.pop_back(); }
    if (!p.empty() && p.back() >= c.index) p.back() = c.index - 1;
    if (!p.empty() && p.back() + 1 == c.index) p.back() = c.index; else { p.push_back(c.index); p.push_back(c.index); }
    b.floor = c.smallest_index;
    file->file_size += header_len + 24 + c.data_len; file->entry_count += 1;
    w.state = RGB_WAL_W_IN_SEQ; w.prev_index = c.index;
  }
  uint32_t np = 0, ne = 0;
  for (uint32_t wn = 0; wn < n_writers; ++wn)
    for (run &b : waiting[wn]) {
      ne += 1;
      for (size_t k = 0; k < b.pairs.size(); k += 2) {
        if (b.pairs[k + 1] < b.floor) continue;
        pairs_out[2 * np] = b.pairs[k] < b.floor ? b.floor : b.pairs[k]; pairs_out[2 * np + 1] = b.pairs[k + 1]; np += 1;
      }
    }
  *n_pairs = np; *n_events = ne;
  return nw;
}
"""


def build_host_loop():
    tmp = tempfile.mkdtemp(prefix="wal_batch_bench_")
    src, lib = os.path.join(tmp, "host_loop.cpp"), os.path.join(tmp, "host_loop.so")
    with open(src, "w") as f:
        f.write(HOST_LOOP)
    subprocess.check_call(["c++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-o", lib, src])
    L = ctypes.CDLL(lib)
    L.host_loop.restype = ctypes.c_uint32
    L.host_loop.argtypes = [ctypes.c_void_p] + [ctypes.c_uint32] + [ctypes.c_void_p] + [ctypes.c_uint32] + [ctypes.c_void_p] * 4 + \
                           [ctypes.c_uint64] + [ctypes.c_void_p] * 5
    return L


KERNELS_ONLY = "--kernels-only" in sys.argv
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
HL = build_host_loop()
eng = engine.RaGpuBatch(1, 1)
stream = torch.cuda.Stream(); sp = stream.cuda_stream
WARM, REPEATS, REPS = 2, 5, 10
N = 65536
UID_LEN = 24


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


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()[:16]


res = []
for label, n_w, size in (("a", 16384, 256), ("a", 16384, 4096), ("c", 1, 256)):
    rng = np.random.default_rng(size + n_w)
    per, total = N // n_w, N * size
    row = {"comparison": label, "commands": N, "writers": n_w, "payload_bytes": size, "repeats": REPEATS}
    # every writer appends `per` consecutive indexes, interleaved in the mailbox; every 64th writer is new to the file
    # and every 97th sends one command ahead of its turn (a resend request, then an ignored command)
    ca = np.zeros(N, dtype=abi.WAL_CMD_DTYPE)
    k = np.arange(N)
    ca["writer"], step = k % n_w, k // n_w
    ca["index"], ca["term"], ca["tid"] = 100 + step, 7, 1 + ca["writer"]
    ca["prev_index"] = ca["index"] - 1
    ahead = (ca["writer"] % 97 == 5) & (step >= per // 2) if per > 1 else np.zeros(N, dtype=bool)
    ca["index"][ahead] += 3; ca["prev_index"][ahead] += 3
    ca["data_len"], ca["data_offset"] = size, n_w * UID_LEN + k.astype(np.uint64) * size
    wa = np.zeros(n_w, dtype=abi.WAL_WRITER_DTYPE)
    wa["state"], wa["prev_index"] = abi.WAL_W_IN_SEQ, 99
    wa["id_ref"] = np.where(np.arange(n_w) % 64 == 0, abi.WAL_NO_ID_REF, np.arange(n_w))
    wa["uid_offset"], wa["uid_len"] = np.arange(n_w) * UID_LEN, UID_LEN
    fa = np.zeros(1, dtype=abi.WAL_FILE_DTYPE)
    fa["max_size"], fa["next_id_ref"] = 1 << 40, n_w
    data_bytes = n_w * UID_LEN + total
    hdr_room = N * 3 + n_w * (2 + UID_LEN)
    d_data = torch.randint(0, 256, (data_bytes + hdr_room + 16,), dtype=torch.uint8, device="cuda")   # the parent's headers ride behind
    uids = d_data[:n_w * UID_LEN].cpu().numpy()
    out_bound, ev_bound, rg_bound = engine.wal_batch_bound(ca, wa, fa, data_bytes)
    d_out = torch.zeros(out_bound, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(16 * N, dtype=torch.uint8, device="cuda")
    d_wout = torch.zeros(32 * n_w, dtype=torch.uint8, device="cuda")
    d_ev = torch.zeros(32 * ev_bound, dtype=torch.uint8, device="cuda")
    d_rg = torch.zeros(16 * rg_bound, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def one_call():
        eng.wal_batch_device(ca, wa, fa, d_data.data_ptr(), data_bytes, d_res.data_ptr(), d_wout.data_ptr(), d_out.data_ptr(),
                             out_bound, d_ev.data_ptr(), ev_bound, d_rg.data_ptr(), rg_bound, d_tot.data_ptr(), 0, sp)

    # the parent's way
    recs = np.zeros(N, dtype=abi.WAL_RECORD_DTYPE)
    hdr = torch.zeros(hdr_room, dtype=torch.uint8).pin_memory()
    recs_pinned = torch.zeros(48 * N, dtype=torch.uint8).pin_memory()
    d_recs = torch.zeros(48 * N, dtype=torch.uint8, device="cuda")
    d_out2 = torch.zeros(out_bound, dtype=torch.uint8, device="cuda")
    verdicts, pairs = np.zeros(N, dtype=np.uint32), np.zeros(2 * N, dtype=np.uint64)
    counts = (ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0))
    state = {}

    def host_way():
        w2, f2 = wa.copy(), fa.copy()
        nw = HL.host_loop(ca.ctypes.data, N, w2.ctypes.data, n_w, uids.ctypes.data, f2.ctypes.data, recs.ctypes.data,
                          hdr.data_ptr(), data_bytes, verdicts.ctypes.data, pairs.ctypes.data, ctypes.byref(counts[0]),
                          ctypes.byref(counts[1]), ctypes.byref(counts[2]))
        end = engine.wal_layout(recs[:nw], 0)
        recs_pinned.numpy()[:48 * nw] = recs[:nw].view(np.uint8)
        with torch.cuda.stream(stream):
            d_recs[:48 * nw].copy_(recs_pinned[:48 * nw], non_blocking=True)
            d_data[data_bytes:data_bytes + hdr_room].copy_(hdr, non_blocking=True)
        eng.wal_frame_device(d_recs.data_ptr(), nw, d_data.data_ptr(), data_bytes + hdr_room, d_out2.data_ptr(), end, 0, 0, sp)
        state.update(nw=nw, end=end, writers=w2, file=f2)

    if KERNELS_ONLY:
        with torch.cuda.stream(stream):
            for _ in range(10):
                one_call(); host_way()
        torch.cuda.synchronize()
        continue
    # interleaved: one way, the other, and again
    t_new = timed(one_call, REPS, WARM)
    t_old = timed(host_way, REPS, WARM)
    t_new2 = timed(one_call, REPS, WARM)
    t_old2 = timed(host_way, REPS, WARM)
    torch.cuda.synchronize()
    tot = d_tot.cpu().numpy().view(abi.WAL_BATCH_TOTAL_DTYPE)[0]
    assert int(tot["status"]) == abi.WAL_BATCH_OK and int(tot["n_written"]) == state["nw"], tot
    out = d_out.cpu().numpy()[:int(tot["out_bytes"])]
    assert int(tot["out_bytes"]) == state["end"] and sha(out) == sha(d_out2.cpu().numpy()[:state["end"]]), "framed bytes differ"
    results = d_res.cpu().numpy().view(abi.WAL_CMD_RESULT_DTYPE)
    assert np.array_equal(results["verdict"] & ~np.uint32(abi.WAL_V_FIRST), verdicts), "verdicts differ from the host loop"
    wout = d_wout.cpu().numpy().view(abi.WAL_WRITER_DTYPE)
    assert wout.tobytes() == state["writers"].tobytes(), "writer rows differ from the host loop"
    n_ev, n_rg = int(tot["n_events"]), int(tot["n_ranges"])
    assert (n_rg, n_ev) == (counts[0].value, counts[1].value)
    ranges = d_rg.cpu().numpy().view(np.uint64)[:2 * n_rg]
    assert np.array_equal(ranges, pairs[:2 * n_rg]), "pairs differ from the host loop"
    row["checked_against"] = "host loop"
    if label == "a":
        from test_wal_batch import Cmd, Writer, check_against, referee
        host = d_data.cpu().numpy()
        cmds = [Cmd(int(c["writer"]), int(c["index"]), int(c["term"]), int(c["prev_index"]), 0, int(c["tid"]),
                    host[int(c["data_offset"]):int(c["data_offset"]) + size].tobytes()) for c in ca]
        ws = [Writer(uids[w * UID_LEN:(w + 1) * UID_LEN].tobytes(), ("in_seq", 99), None if w % 64 == 0 else w)
              for w in range(n_w)]
        ref = referee(cmds, ws, 0, 0, n_w, 1 << 40, 0)
        events = d_ev.cpu().numpy().view(abi.WAL_EVENT_DTYPE)[:n_ev]
        check_against(ref, (tot, results, wout, out, events, ranges.reshape(-1, 2)), n_w)
        row["checked_against"] = "host loop and referee"
        row["verdicts"] = {name: int((results["verdict"] & abi.WAL_V_MASK == v).sum())
                           for name, v in (("write", 1), ("drop", 2), ("ignore", 3), ("resend", 4))}
    row["out_sha256_16"] = sha(out)
    for name, t in (("one_call", t_new), ("host_loop_and_frame", t_old), ("one_call_again", t_new2),
                    ("host_loop_and_frame_again", t_old2)):
        row[name + "_us"], row[name + "_us_min"], row[name + "_us_max"] = t
    row["host_way_vs_one_call"] = t_old[0] / t_new[0]                                # > 1: the one call is faster
    row["faster_beyond_spread"] = bool(max(t_new[2], t_new2[2]) < min(t_old[1], t_old2[1]))
    row["one_call_GBps"] = total / 1e9 / (t_new[0] * 1e-6)
    res.append(row)
    print(json.dumps(row), flush=True)
    del d_data, d_out, d_out2, d_res, d_wout, d_ev, d_rg

if not KERNELS_ONLY:
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", "wal_batch_bench.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
eng.close()
