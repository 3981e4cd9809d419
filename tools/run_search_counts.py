#!/usr/bin/env python3
"""Dependent run-table round trips of the snapshot_written lanes, counted over STATE on the CPU emulation (no GPU): the
closed-loop generator with bench.py's seed, aged, then sampled tick by tick.  For every snapshot_written message whose
find_run reaches the in-memory runs (index + 1 inside the range, below the two runs mirrored in the hot row, three runs
and more) the script replays both searches on the downloaded table -- the walk (run_search: newest first, one dependent
step per run) and the bisection (run_search_canonical: the newest in-memory run and run 1 asked for together, then
halving) -- and prints mean and maximum per lane and the maximum per 64 consecutive messages of the class.
"Canonical" is judged from the table itself (starts and terms strictly increasing, run 0 at first_index); the row's
bit can only be clear more often.   usage: python tools/run_search_counts.py [groups] [ageing ticks] [sampled ticks]"""
import os, subprocess, sys, tempfile
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
from ra_amd import abi, engine, workload as W

G = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
AGE = int(sys.argv[2]) if len(sys.argv) > 2 else 512
T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
N, SEED = 5, 0x5EED0003


def build(tmp):
    """The emulation library as tests/conftest.py builds it (group size 5 only)."""
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


def walk(starts, top, idx):
    """run_search: dependent steps (one per run examined), run found."""
    for steps, k in enumerate(range(top, -1, -1), 1):
        if idx >= starts[k]:
            return steps, k
    return top + 1, -1


def bisect(starts, top, idx):
    """run_search_canonical without a term: dependent round trips, run found."""
    if idx >= starts[top]:
        return 1, top
    if top == 0:
        return 1, -1
    if idx < starts[1]:
        return 1, 0                                    # run 0 starts at first_index <= idx: no further load
    k, hi, trips = 1, top, 1
    while hi - k > 1:
        mid = (k + hi) >> 1
        trips += 1
        if idx >= starts[mid]:
            k = mid
        else:
            hi = mid
    return trips, k


with tempfile.TemporaryDirectory() as tmp:
    engine.LIB_PATH, engine._lib = build(tmp), None
    S, tb = G * N, G * N * 64
    eng = engine.RaGpuBatch(G, N, max_runs=16, ring_slots=1, ring_capacity=64)
    eng.set_state(0, W.initial_states(G, N, SEED))
    dm, dd = np.zeros(tb, dtype=np.uint8), np.zeros(tb, dtype=np.uint8)
    dr = np.zeros(S * 4 * 56, dtype=np.uint8)
    dn = np.zeros(1, dtype=np.uint32)
    lanes = reach = noncanon = 0
    w_steps, b_trips, w_wave, b_wave = [], [], [], []
    for t in range(AGE + T):
        eng.synth_tick_buckets_device(SEED, t, dm.ctypes.data, 0, dn.ctypes.data, 0)
        eng.synchronize()
        if t >= AGE:
            st = eng.get_state()
            m = dm[:int(dn[0]) * 64].view(abi.MSG_DTYPE)
            m = m[m["kind"] == abi.MSG_SNAPSHOT_WRITTEN]
            per = []
            for srv, idx in zip(m["server"], m["a"]):
                r = st[srv]
                n, first, li = int(r["n_runs"]), int(r["first_index"]), int(r["last_index"])
                starts, terms = [int(x) for x in r["run_start"][:n]], [int(x) for x in r["run_term"][:n]]
                lanes += 1
                nf = int(idx) + 1
                if not (first <= li and first <= idx < li) or n < 3 or nf >= starts[n - 2]:
                    per.append((0, 0))
                    continue
                reach += 1
                canon = starts[0] <= first and all(starts[k] < starts[k + 1] and terms[k] < terms[k + 1] for k in range(n - 1))
                ws, wk = walk(starts, n - 3, nf)
                bs, bk = bisect(starts, n - 3, nf) if canon else (ws, wk)
                assert wk == bk, (starts, nf, wk, bk)
                noncanon += 0 if canon else 1
                w_steps.append(ws); b_trips.append(bs)
                per.append((ws, bs))
            for i in range(0, len(per), 64):
                w_wave.append(max(p[0] for p in per[i:i + 64])); b_wave.append(max(p[1] for p in per[i:i + 64]))
        eng.synth_apply_tick_device(dm.ctypes.data, S, dd.ctypes.data, dr.ctypes.data)
        eng.synchronize()
    w, b = np.array(w_steps), np.array(b_trips)
    print(f"{G} groups x {N}, {AGE} ageing ticks, {T} sampled ticks: {lanes} snapshot_written lanes, {reach} reach the in-memory runs "
          f"({100.0 * reach / max(lanes, 1):.1f} %), {noncanon} of them on tables that are not canonical")
    print(f"  walk      : dependent loads per reaching lane mean {w.mean():.2f} max {w.max()}; per 64 messages: mean of the maxima {np.mean(w_wave):.2f}, max {max(w_wave)}")
    print(f"  bisection : dependent loads per reaching lane mean {b.mean():.2f} max {b.max()}; per 64 messages: mean of the maxima {np.mean(b_wave):.2f}, max {max(b_wave)}")
    print("  walk histogram (steps 1..):", np.bincount(w)[1:].tolist())
    print("  bisection histogram (trips 1..):", np.bincount(b)[1:].tolist())
    eng.close()
