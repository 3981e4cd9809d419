#!/usr/bin/env python3
"""The decisions a tick still stores as 64-byte records, counted on the CPU emulation (no GPU): the closed-loop generator
with bench.py's seed, aged, then sampled tick by tick.  Every sampled decision is classified by the encoder of the
header's comment (include/ra_gpu_batch.h, "Compact decisions") as abi.compact_forms restates it on the host; the
records it leaves full are counted by kind, by `flags & ~plain`, by which of the words 2..7 are non-zero, by n_rpcs and by the aux fields
(invariant, heartbeat_to, cancel_backoff).  The stream the emulated kernels wrote is checked against the same
classification, so the table is also a test of the encoder that is built.
usage: python tools/decision_form_counts.py [groups] [ageing ticks] [sampled ticks] [file for the full records (.npy)]"""
import os, subprocess, sys, tempfile
from collections import Counter
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
from ra_amd import abi, engine, workload as W

G = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
AGE = int(sys.argv[2]) if len(sys.argv) > 2 else 512
T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
DUMP = sys.argv[4] if len(sys.argv) > 4 else None
N, SEED = 5, 0x5EED0003
WORDS = ("reply_term", "reply_next_index", "reply_last_index", "reply_last_term", "commit_index", "last_applied")


def build(tmp):
    """The emulation library as tests/conftest.py builds it; RGB_EMU_LIB names one that is built already."""
    if os.environ.get("RGB_EMU_LIB"):
        return os.environ["RGB_EMU_LIB"]
    clang = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else "clang++"
    nat = os.path.join(root, "tests", "native")
    flags = ["-std=c++17", "-O1", "-fPIC", "-DRGB_EMU_FULL_API", "-Wno-unknown-pragmas", "-Wno-pass-failed",
             "-Wno-unused-function", "-Wno-unused-variable", "-I", os.path.join(nat, "fake_hip"), "-I", os.path.join(root, "include")]
    units = [("api", "api_on_cpu.cpp", []), ("wal", "wal_on_cpu.cpp", []), ("comm", "comm_on_cpu.cpp", []),
             ("dispatch", "kernel_dispatch_on_cpu.cpp", [])]
    units += [("kernel_N%d" % n, "kernel_on_cpu.cpp", ["-DRGB_EMU_ONLY_N=%d" % n]) for n in range(1, 9)]
    procs = [subprocess.Popen([clang, "-x", "c++", "-c"] + flags + more + ["-o", os.path.join(tmp, name + ".o"), os.path.join(nat, src)])
             for name, src, more in units]
    assert all(p.wait() == 0 for p in procs)
    out = os.path.join(tmp, "libkernels_on_cpu.so")
    subprocess.check_call([clang, "-shared", "-Wl,-Bsymbolic", "-o", out] + [os.path.join(tmp, name + ".o") for name, _, _ in units])
    return out


with tempfile.TemporaryDirectory() as tmp:
    engine.LIB_PATH, engine._lib = build(tmp), None
    S, tb = G * N, G * N * 64
    eng = engine.RaGpuBatch(G, N, max_runs=16, ring_slots=1, ring_capacity=64)
    eng.set_state(0, W.initial_states(G, N, SEED))
    dm, dd = np.zeros(tb, dtype=np.uint8), np.zeros(tb, dtype=np.uint8)
    dr = np.zeros(S * 4 * 56, dtype=np.uint8)
    dn = np.zeros(1, dtype=np.uint32)
    total = stored_compact = 0
    by_form, by_kind, by_class, full = Counter(), Counter(), Counter(), []
    for t in range(AGE + T):
        eng.synth_tick_buckets_device(SEED, t, dm.ctypes.data, 0, dn.ctypes.data, 0)
        eng.synchronize()
        eng.synth_apply_tick_device(dm.ctypes.data, S, dd.ctypes.data, dr.ctypes.data)
        eng.synchronize()
        if t < AGE:
            continue
        n = int(dn[0])
        raw = dd[:n * 64].view(abi.DECISION_DTYPE)
        d = abi.expand_decisions(raw)
        d = d[d["kind"] != abi.MSG_NOP]
        stored = (raw["flags"][raw["kind"] != abi.MSG_NOP] & abi.F_COMPACT) != 0
        total += len(d); stored_compact += int(stored.sum())
        form = abi.compact_forms(d)
        assert np.array_equal(form != 0, stored), "the emulated kernels and abi.compact_forms disagree on what is compact"
        for f, c in zip(*np.unique(form, return_counts=True)):
            by_form[abi.COMPACT_FORM_NAMES[int(f)]] += int(c)
        f = d[form == 0]
        full.append(f)
        shape = f["flags"] & ~np.uint32(abi.F_COMPACT_PLAIN)
        words = sum(((f[w] != 0).astype(np.uint32) << k) for k, w in enumerate(WORDS))
        aux = (f["invariant"] != 0) | ((f["heartbeat_to"] != 0) << 1) | ((f["cancel_backoff"] != 0) << 2)
        for key, c in Counter(zip(f["kind"].tolist(), shape.tolist(), words.tolist(), (f["n_rpcs"] != 0).tolist(),
                                  aux.tolist())).items():
            by_class[key] += c
        for k, c in zip(*np.unique(f["kind"], return_counts=True)):
            by_kind[int(k)] += int(c)
    eng.close()

n_full = sum(by_kind.values())
print(f"{G} groups x {N}, {AGE} ageing ticks, {T} sampled ticks: {total / T:.0f} decisions per tick, "
      f"{stored_compact / T:.0f} compact, {n_full / T:.0f} full ({100.0 * n_full / total:.1f} %); "
      f"decision bytes per tick {(64 * n_full + 32 * stored_compact) / T:.0f}")
print("compact, per tick, by form: " + ", ".join(f"{k} {v / T:.0f}" for k, v in sorted(by_form.items()) if k != "full"))
print("full records per tick by kind: " + ", ".join(f"{k}: {v / T:.0f}" for k, v in sorted(by_kind.items())))
print("full records per tick by (kind, flags & ~plain, non-zero words 2..7 as w2 = bit 0, n_rpcs != 0, "
      "aux: invariant = 1, heartbeat_to = 2, cancel_backoff = 4), classes of 0.2 % and more:")
print("| kind | flags & ~plain | words | rpcs | aux | per tick | share | cumulative |")
print("|---|---|---|---|---|---|---|---|")
cum = 0
for (kind, shape, words, rp, aux), c in by_class.most_common():
    cum += c
    if c * 500 >= n_full:
        print(f"| {kind} | {shape:#x} | {words:06b} | {int(rp)} | {aux} | {c / T:.0f} | {100.0 * c / n_full:.1f} % | {100.0 * cum / n_full:.1f} % |")
if DUMP:
    np.save(DUMP, np.concatenate(full))
