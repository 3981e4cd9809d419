#!/usr/bin/env python3
"""rgb_submit against rgb_submit_raw and begin / fill in place / commit, on one box in one process.

Legs (each its own context, all from the same state, fed the same batches, interleaved round trip by round trip):
    a1, a2  rgb_submit + rgb_collect_view on the PARENT commit's library (--parent-lib, built to a side directory):
            the baseline, twice -- the difference between the two is the spread a real difference has to beat
    b       the same calls on this tree's library: must sit inside that spread (the existing path did not move)
    c       rgb_submit_raw (max_rounds = the rounds the shape has)
    c4      rgb_submit_raw with max_rounds = 4 on the single-round shapes: what the three empty round launches cost
    d       rgb_submit_begin / fill the pinned slot in place / rgb_submit_commit
Shapes: single-round batches of 64, 1 024, 4 096 and 16 384 messages, the ~15.5 k four-round batch of
tools/host_path_ab.py, and 131 072-message batches pipelined three deep from one thread.
Per leg and shape: host time inside the submit call(s) per message, the round trip's p50, decisions per second; a
digest of every decision and rpc record handed out, compared between the legs.  One JSON line on stdout (--out FILE
writes it there as well).  Without --parent-lib the a-legs are left out.
    python tools/submit_raw_bench.py --parent-lib ra_amd/csrc/variants/parent.so --out profiles/submit_raw_bench.json
What the prepare kernels and the round launches take on the device comes from a trace of its own, one leg and one shape:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/submit_raw_bench.py --only-shape four_rounds --only-legs c"""
import argparse, hashlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from ra_amd import abi, engine, workload as W

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--trips", type=int, default=300)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--groups", type=int, default=65536)
ap.add_argument("--big", type=int, default=131072)
ap.add_argument("--only-shape", default=None, help="one shape only, no pipelined part (a kernel trace of one leg: see below)")
ap.add_argument("--only-legs", default=None, help="comma-separated subset of the legs")
args = ap.parse_args()

G, N, seed = args.groups, 5, 0x5EED0003
S = G * N
B = args.big


def bind(path):
    """ra_amd.engine bound to another build for the engines created while it is (a context keeps its library)."""
    saved = (engine.LIB_PATH, engine._lib, os.environ.get("RGB_LIB"))
    engine.LIB_PATH, engine._lib = path, None
    os.environ["RGB_LIB"] = path                    # (an older build may lack the newest exports)
    engine.lib()
    return saved


def unbind(saved):
    engine.LIB_PATH, engine._lib = saved[0], saved[1]
    if saved[2] is None:
        os.environ.pop("RGB_LIB", None)
    else:
        os.environ["RGB_LIB"] = saved[2]


def make_engine():
    return engine.RaGpuBatch(G, N, max_runs=16, ring_capacity=B, ring_slots=4)


engine.lib()
legs = {}
if args.parent_lib:
    saved = bind(os.path.abspath(args.parent_lib))
    legs["a1"] = make_engine(); legs["a2"] = make_engine()
    unbind(saved)
for name in ("b", "c", "c4", "d"):
    legs[name] = make_engine()
if args.only_legs:
    keep = set(args.only_legs.split(",")) | {"b"}          # (leg b's context also generates the workload)
    for k in [k for k in legs if k not in keep]:
        legs.pop(k).close()

st0 = W.initial_states(G, N, seed)
gen = legs["b"]
gen.set_state(0, st0)
stream = torch.cuda.Stream(); sp = stream.cuda_stream
dm = torch.zeros(S * 64, dtype=torch.uint8, device="cuda"); dd = torch.zeros(S * 64, dtype=torch.uint8, device="cuda")
dn = torch.zeros(1, dtype=torch.int32, device="cuda")
ticks = []
for t in range(8):
    with torch.cuda.stream(stream):
        gen.synth_tick_device(seed, t, dm.data_ptr(), 0, dn.data_ptr(), sp)
        gen.synth_apply_tick_device(dm.data_ptr(), S, dd.data_ptr(), 0, sp)
    torch.cuda.synchronize()
    ticks.append(dm[:int(dn.item()) * 64].cpu().numpy().view(abi.MSG_DTYPE).copy())
del dm, dd

shapes = [(f"one_round_{n}", ticks[0][:n].copy(), 1) for n in (64, 1024, 4096, 16384)]
shapes.append(("four_rounds", np.concatenate([m[m["server"] < 1024 * N] for m in ticks[:4]]), 4))
if args.only_shape:
    shapes = [s for s in shapes if s[0] == args.only_shape]
    if args.only_legs and "b" not in args.only_legs.split(","):
        legs.pop("b").close()


def submit_of(name, eng, rounds):
    """-> f(msgs) returning the seconds spent inside the library's submit call(s)"""
    if name in ("a1", "a2", "b"):
        def f(m):
            t0 = time.perf_counter(); eng.submit(m); return time.perf_counter() - t0
    elif name in ("c", "c4"):
        R = 4 if name == "c4" else rounds

        def f(m):
            t0 = time.perf_counter(); eng.submit_raw(m, max_rounds=R); return time.perf_counter() - t0
    else:
        def f(m):
            t0 = time.perf_counter(); buf, slot = eng.submit_begin(rounds); t1 = time.perf_counter()
            buf[:len(m)] = m                        # the producer's own fill: not library time
            t2 = time.perf_counter(); eng.submit_commit(slot, len(m), 0); return (t1 - t0) + (time.perf_counter() - t2)
    return f


def p50(v):
    return sorted(v)[len(v) // 2]


out = {"groups": G, "members": N, "trips": args.trips, "parent_lib": args.parent_lib, "shapes": {}}
for label, msgs, rounds in shapes:
    use = [k for k in legs if not (k == "c4" and rounds != 1)]
    fs = {k: submit_of(k, legs[k], rounds) for k in use}
    for k in use:
        legs[k].set_state(0, st0)
    rt = {k: [] for k in use}; sub = {k: [] for k in use}; dig = {k: hashlib.sha256() for k in use}
    for i in range(args.warmup + args.trips):
        for k in use:                                # interleaved: every leg sees the same minute of the box
            eng = legs[k]
            t0 = time.perf_counter()
            ts = fs[k](msgs)
            d, r, _, slot = eng.collect_view()
            t1 = time.perf_counter()
            dig[k].update(d.tobytes()); dig[k].update(r.tobytes())
            eng.release(slot)
            if i >= args.warmup:
                rt[k].append(t1 - t0); sub[k].append(ts)
    res = {}
    for k in use:
        res[k] = {"submit_ns_per_message": round(p50(sub[k]) / len(msgs) * 1e9, 2),
                  "round_trip_us_p50": round(p50(rt[k]) * 1e6, 1),
                  "round_trip_us_p10": round(sorted(rt[k])[len(rt[k]) // 10] * 1e6, 1),
                  "decisions_per_s": round(len(msgs) / p50(rt[k])),
                  "digest": dig[k].hexdigest()[:16]}
    out["shapes"][label] = {"messages": int(len(msgs)), "rounds": rounds, "legs": res,
                            "digests_equal": len({v["digest"] for v in res.values()}) == 1}

# ---- 131 072-message batches from one thread, three ahead ----
big = [m[i:i + B] for m in ticks for i in range(0, len(m), B)] if not args.only_shape else []
use = [k for k in legs if k != "c4"]
res = {k: {"rates": [], "submit": []} for k in use}
for rep in range(4 if big else 0):                   # (rep 0 warms up and gives the digest)
    for k in use:
        eng = legs[k]; f = submit_of(k, eng, 1)
        eng.set_state(0, st0)
        h = hashlib.sha256(); pending = nd = 0; ts = 0.0
        t0 = time.perf_counter()
        for m in big:
            while pending >= 3:
                d, r, _, slot = eng.collect_view()
                if rep == 0:
                    h.update(d.tobytes()); h.update(r.tobytes())
                eng.release(slot); pending -= 1
            ts += f(m); pending += 1; nd += len(m)
        while pending:
            d, r, _, slot = eng.collect_view()
            if rep == 0:
                h.update(d.tobytes()); h.update(r.tobytes())
            eng.release(slot); pending -= 1
        el = time.perf_counter() - t0
        if rep == 0:
            res[k]["digest"] = h.hexdigest()[:16]
        else:
            res[k]["rates"].append(nd / el); res[k]["submit"].append(ts / nd)
if big:
    out["shapes"][f"pipelined_{B}"] = {
      "messages": int(sum(len(m) for m in big)), "batches": len(big),
      "legs": {k: {"submit_ns_per_message": round(min(v["submit"]) * 1e9, 2),
                   "decisions_per_s": round(max(v["rates"])), "decisions_per_s_all": [round(x) for x in v["rates"]],
                   "digest": v["digest"]} for k, v in res.items()},
      "digests_equal": len({v["digest"] for v in res.values()}) == 1}
for e in legs.values():
    e.close()
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
