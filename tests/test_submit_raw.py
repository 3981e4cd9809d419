"""rgb_submit_raw / rgb_submit_begin / rgb_submit_commit: a batch whose validation, sub-tick rounds and bucket order
run on the device (ra_amd/csrc/rgb_prepare.hip) instead of on the submitting thread.

The sequential checker (oracle.Oracle: one message at a time, in submission order) is the referee everywhere; rgb_submit
on a second engine is the byte-for-byte comparison the raw path must not differ from.  Every check is a plain function
of an engine module: the CPU tests run it on the emulated library (tests/native: the product's sources on a block
emulation), the `-m gpu` twins on the device."""
import os
import subprocess
import threading

import numpy as np
import pytest

import fuzz
from emu_schedule import PERMUTED_SCHEDULES, schedule
from ra_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu_engine():
    from ra_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build()    # a fresh checkout on the GPU box: hipcc is there, the .so is not in git
    engine.lib()          # raises if the HIP library is missing: no fallback
    return engine


# ------------------------------------------------------------------------------------------ helpers

def multi_round_batch(rng, state, n_members, rounds, frac=0.8):
    """`rounds` ticks built like fuzz.random_msgs (at most one message per server each, NOP records included),
    concatenated and shuffled: at most `rounds` messages per server, in any order."""
    msgs = np.concatenate([fuzz.random_msgs(rng, state, n_members, frac=frac) for _ in range(rounds)])
    rng.shuffle(msgs)
    return msgs


def fill_and_commit(gpu, msgs, tick, max_rounds):
    buf, slot = gpu.submit_begin(max_rounds)
    assert len(buf) == gpu.raw_capacity(max_rounds)
    buf[:len(msgs)] = msgs                      # written in place, submission order
    gpu.submit_commit(slot, len(msgs), tick)


def expect_error(engine, fn, code):
    with pytest.raises(engine.RgbError) as e:
        fn()
    assert e.value.code == code, (e.value.code, code)


def assert_state_equal(tag, got, want):
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()]
        diff = [n for n in got.dtype.names if np.any(got[bad[0]][n] != want[bad[0]][n])]
        raise AssertionError(f"{tag}: state of server {bad[0]} differs in {diff} ({len(bad)} servers differ)")


# ------------------------------------------------------------------------------------------ 1. differential

def check_differential(engine, O, n_members, rounds, groups, seed, batches=3):
    """The same batches through rgb_submit (engine A), rgb_submit_raw (B) and begin / fill in place / commit with
    rgb_collect_view (C), from equal random states: decisions and rpc records byte-identical between the three and
    equal to the checker's, the states too.  Sizes: one message, exactly raw_capacity, and whatever the draw gives."""
    rng = np.random.default_rng(seed)
    st = fuzz.random_states(rng, groups, n_members, max_runs=6)
    cpu = O.Oracle(groups, n_members, max_runs=16)
    cpu.set_state(0, st)
    # a slot that a batch of `rounds` ticks of ~0.8 messages per server each overfills: the second batch is cut to
    # exactly raw_capacity
    target = int(0.6 * groups * n_members * rounds)
    ring_capacity = sum(target // (r + 1) for r in range(rounds))
    mk = lambda: engine.RaGpuBatch(groups, n_members, ring_capacity=ring_capacity, ring_slots=2, max_runs=16)
    with mk() as a, mk() as b, mk() as c:
        for g in (a, b, c):
            g.set_state(0, st)
        cap = b.raw_capacity(rounds)
        bounds = sum(cap // (r + 1) for r in range(rounds))
        assert cap >= target and bounds <= ring_capacity < sum((cap + 1) // (r + 1) for r in range(rounds)), (cap, rounds, ring_capacity)
        nops = 0
        for k in range(batches):
            msgs = multi_round_batch(rng, cpu.get_state(), n_members, rounds)
            if k == 0:
                msgs = msgs[:1]
            elif k == 1:
                assert len(msgs) >= cap, (len(msgs), cap)
                msgs = msgs[:cap]                                 # a full slot: every round region up to its bound
            else:
                msgs = msgs[:min(len(msgs), cap)]
            nops += int((msgs["kind"] == abi.MSG_NOP).sum())
            do, ro = cpu.step(msgs)
            a.submit(msgs, tick=k)
            da, ra, _ = a.collect()
            b.submit_raw(msgs, tick=k, max_rounds=rounds)
            db, rb, tb = b.collect()
            fill_and_commit(c, msgs, k, rounds)
            dc, rc, tc, slot = c.collect_view()
            tag = f"N={n_members} rounds={rounds} batch {k} ({len(msgs)} messages)"
            assert tb == k and tc == k
            assert db.tobytes() == da.tobytes(), tag + ": raw decisions differ from rgb_submit's"
            assert rb.tobytes() == ra.tobytes(), tag + ": raw rpc records differ from rgb_submit's"
            assert dc.tobytes() == da.tobytes() and rc.tobytes() == ra.tobytes(), tag + ": begin/commit + view"
            c.release(slot)
            assert db.tobytes() == do.tobytes(), tag + ": decisions differ from the checker's"
            assert fuzz.sort_rpcs(rb.copy()).tobytes() == fuzz.sort_rpcs(ro).tobytes(), tag + ": rpcs vs checker"
            sa, want = a.get_state(), cpu.get_state()
            assert_state_equal(tag + " (rgb_submit)", sa, want)
            assert_state_equal(tag + " (rgb_submit_raw)", b.get_state(), want)
            assert_state_equal(tag + " (begin/commit)", c.get_state(), want)
        assert nops > 0, "no NOP record was mixed in"
    cpu.close()


# N in {1, 2, 3, 5, 7, 8}, 1 to 8 rounds per server
DIFF_CASES = [(1, 1, 300, 11), (2, 2, 150, 12), (3, 3, 120, 13), (5, 4, 64, 14), (7, 5, 40, 15), (8, 8, 24, 16),
              (5, 6, 48, 17), (3, 7, 64, 18), (5, 1, 128, 19), (8, 2, 60, 20)]


@pytest.mark.parametrize("n_members,rounds,groups,seed", DIFF_CASES)
def test_raw_equals_submit_and_checker(emulated_engine, oracle_lib, n_members, rounds, groups, seed):
    check_differential(emulated_engine, oracle_lib, n_members, rounds, groups, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("n_members,rounds,groups,seed", DIFF_CASES)
def test_gpu_raw_equals_submit_and_checker(gpu_engine, oracle_lib, n_members, rounds, groups, seed):
    check_differential(gpu_engine, oracle_lib, n_members, rounds, groups, seed)
    # the same at a size where every round is worth a real launch
    check_differential(gpu_engine, oracle_lib, n_members, rounds, groups * 16, seed + 100)


# ------------------------------------------------------------------------------------------ 2. refusals

def _rec(**kw):
    r = np.zeros(1, dtype=abi.MSG_DTYPE)
    for k, v in kw.items():
        r[k] = v
    return r[0]


def bad_records(n_servers):
    """One record per clause of validate_msg (rgb_api.hip), then the written event with a range list."""
    U = abi.UNDEF_INT
    return [
        ("kind", _rec(server=0, kind=abi.MSG_TRANSFER_LEADERSHIP + 1), abi.E_INVAL),
        ("server", _rec(server=n_servers, kind=abi.MSG_AER), abi.E_INVAL),
        ("from", _rec(server=1, kind=abi.MSG_AER_REPLY, **{"from": abi.MAX_MEMBERS}), abi.E_INVAL),
        ("aer_run0", _rec(server=1, kind=abi.MSG_AER, n_entries=2, n_run0=3), abi.E_INVAL),
        ("written_range", _rec(server=1, kind=abi.MSG_WRITTEN, a=9, b=8), abi.E_INVAL),
        ("seq2_order", _rec(server=1, kind=abi.MSG_WRITTEN, flags=abi.MF_SEQ2, run0_term=5, run1_term=4, a=9, b=9), abi.E_INVAL),
        ("seq2_undef", _rec(server=1, kind=abi.MSG_WRITTEN, flags=abi.MF_SEQ2, run0_term=5, run1_term=U, a=9, b=9), abi.E_INVAL),
        ("seq2_adjacent", _rec(server=1, kind=abi.MSG_WRITTEN, flags=abi.MF_SEQ2, run0_term=5, run1_term=8, a=9, b=9), abi.E_INVAL),
        ("seqx_without_seq2", _rec(server=1, kind=abi.MSG_WRITTEN, flags=abi.MF_SEQX, a=9, b=9), abi.E_INVAL),
        ("seqx", _rec(server=1, kind=abi.MSG_WRITTEN, flags=abi.MF_SEQ2 | abi.MF_SEQX, run0_term=5, run1_term=6, a=9, b=9,
                      c=0, n_entries=1), abi.E_INVAL),
    ]


def check_refusals(engine, O, flags=0, groups=24, n_members=3, seed=31):
    """Every refused batch: the documented code exactly once -- from collect, from collect behind a peek (which sizes
    the batch as empty) and from collect_view in turn --, nothing applied (checksum and state as before), and the next
    valid batch on the same servers equal to the checker's, which never saw the refused one: the per-server scratch of
    the prepare kernels was left clean."""
    rng = np.random.default_rng(seed)
    S = groups * n_members
    st = fuzz.random_states(rng, groups, n_members, max_runs=6)
    cpu = O.Oracle(groups, n_members, max_runs=16)
    cpu.set_state(0, st)
    R = 3
    with engine.RaGpuBatch(groups, n_members, ring_capacity=1024, ring_slots=2, max_runs=16, flags=flags) as gpu:
        gpu.set_state(0, st)
        cases = []
        for name, rec, code in bad_records(S):
            for where in ("first", "middle", "last"):
                cases.append((name, where, rec, code))
        cases.append(("too_many_rounds", "last", None, abi.E_UNSUPPORTED))
        # an invalid record BEHIND a server that is already over max_rounds: the input error wins
        cases.append(("aer_run0", "behind too_many_rounds", {n: r for n, r, _ in bad_records(S)}["aer_run0"], abi.E_INVAL))
        ways = ("collect", "peek", "view")
        for k, (name, where, rec, code) in enumerate(cases):
            good = multi_round_batch(rng, cpu.get_state(), n_members, 2)
            if rec is None or where == "behind too_many_rounds":
                # max_rounds + 1 messages for one server (every one of them valid)
                srv = int(good["server"][good["kind"] != abi.MSG_NOP][0])
                extra = np.zeros(R + 1, dtype=abi.MSG_DTYPE)
                extra["server"], extra["kind"] = srv, abi.MSG_PIPELINE_RPCS
                batch = np.concatenate([good[good["server"] != srv], extra])
                if rec is not None:
                    batch = np.concatenate([batch, np.array([rec], dtype=abi.MSG_DTYPE)])
            else:
                at = {"first": 0, "middle": len(good) // 2, "last": len(good)}[where]
                batch = np.concatenate([good[:at], np.array([rec], dtype=abi.MSG_DTYPE), good[at:]])
            before_sum, before = gpu.state_checksum(), gpu.get_state()
            if k % 2:
                gpu.submit_raw(batch, tick=k, max_rounds=R)
            else:
                fill_and_commit(gpu, batch, k, R)
            way = ways[k % 3]
            tag = f"{name} at {where} via {way}"
            if way == "peek":
                n, nr = C_u32(), C_u32()
                assert gpu._L.rgb_peek(gpu._h, byref(n), byref(nr)) == abi.OK, tag
                assert (n.value, nr.value) == (0, 0), tag + ": a refused batch is sized as empty"
            with pytest.raises(engine.RgbError) as e:
                gpu.collect_view() if way == "view" else gpu.collect()
            assert e.value.code == code, f"{tag}: rc {e.value.code}, want {code}"
            expect_error(engine, gpu.collect, abi.E_EMPTY)                     # .. exactly once: the ring moved on
            assert gpu.in_flight == 0
            assert gpu.state_checksum() == before_sum, tag + ": the refused batch changed the state checksum"
            assert_state_equal(tag + ": the refused batch applied something", gpu.get_state(), before)
            # the batch behind it: valid, the same servers
            do, ro = cpu.step(good)
            dg, rg = gpu.step_raw(good, max_rounds=R)
            assert dg.tobytes() == do.tobytes(), tag + ": the batch behind the refused one"
            assert fuzz.sort_rpcs(rg).tobytes() == fuzz.sort_rpcs(ro).tobytes(), tag
            assert_state_equal(tag + ": behind the refused batch", gpu.get_state(), cpu.get_state())
        # a refused batch with batches behind it IN FLIGHT: they run normally
        good1 = multi_round_batch(rng, cpu.get_state(), n_members, 2)
        bad = np.concatenate([good1, np.array([bad_records(S)[1][1]], dtype=abi.MSG_DTYPE)])
        gpu.submit_raw(bad, tick=900, max_rounds=R)
        gpu.submit_raw(good1, tick=901, max_rounds=R)
        expect_error(engine, gpu.collect, abi.E_INVAL)
        do, ro = cpu.step(good1)
        dg, rg, tick = gpu.collect()
        assert tick == 901 and dg.tobytes() == do.tobytes()
        assert_state_equal("in flight behind a refused batch", gpu.get_state(), cpu.get_state())
    cpu.close()


def C_u32():
    import ctypes
    return ctypes.c_uint32(0)


def byref(x):
    import ctypes
    return ctypes.byref(x)


def check_synchronous_errors(engine, flags=0):
    """What the host still checks in the call itself: sizes and the slot's state."""
    G, N = 16, 3
    with engine.RaGpuBatch(G, N, ring_capacity=64, ring_slots=2, flags=flags) as gpu:
        nop = np.zeros(4, dtype=abi.MSG_DTYPE)
        # the capacity rule: the largest n whose round regions fit the slot
        for R in range(1, 9):
            cap = gpu.raw_capacity(R)
            assert sum(cap // (r + 1) for r in range(R)) <= 64 < sum((cap + 1) // (r + 1) for r in range(R))
        assert gpu.raw_capacity(1) == 64 and gpu.raw_capacity(0) == gpu.raw_capacity(4) and gpu.raw_capacity(9) == 0
        expect_error(engine, lambda: gpu.submit_begin(9), abi.E_INVAL)
        expect_error(engine, lambda: gpu.submit_raw(nop, max_rounds=9), abi.E_INVAL)
        # n > cap
        cap = gpu.raw_capacity(4)
        expect_error(engine, lambda: gpu.submit_raw(np.zeros(cap + 1, dtype=abi.MSG_DTYPE), max_rounds=4), abi.E_INVAL)
        assert gpu.in_flight == 0
        buf, slot = gpu.submit_begin(4)
        assert len(buf) == cap
        expect_error(engine, lambda: gpu.submit_commit(slot, cap + 1, 0), abi.E_INVAL)
        # .. the slot stays begun: n = 0 gives it back, and it collects as an empty batch with its tick
        gpu.submit_commit(slot, 0, 77)
        d, r, tick = gpu.collect()
        assert (len(d), len(r), tick) == (0, 0, 77)
        # commit of a slot that was not begun (twice the same slot; a slot the ring does not have)
        expect_error(engine, lambda: gpu.submit_commit(slot, 0, 0), abi.E_STATE)
        expect_error(engine, lambda: gpu.submit_commit(99, 0, 0), abi.E_INVAL)
        if not flags & abi.CFG_SUBMIT_TRAINS:
            # begin on a full ring (two slots: one begun, one published)
            buf, slot = gpu.submit_begin(1)
            buf2, slot2 = gpu.submit_begin(1)
            assert slot2 != slot
            expect_error(engine, lambda: gpu.submit_begin(1), abi.E_FULL)
            expect_error(engine, lambda: gpu.submit(nop), abi.E_FULL)
            buf[:4] = nop
            gpu.submit_commit(slot, 4, 1)
            gpu.submit_commit(slot2, 0, 2)
            expect_error(engine, lambda: gpu.submit_begin(1), abi.E_FULL)      # published, not collected: still full
            d, _, tick = gpu.collect()
            assert (len(d), tick) == (4, 1) and np.all(d["reply_to"] == abi.NONE) and np.all(d["flags"] == 0)
            d, _, tick = gpu.collect()
            assert (len(d), tick) == (0, 2)
        expect_error(engine, gpu.collect, abi.E_EMPTY)


def test_refused_batches_are_per_batch_results(emulated_engine, oracle_lib):
    check_refusals(emulated_engine, oracle_lib)


def test_synchronous_errors(emulated_engine):
    check_synchronous_errors(emulated_engine)


@pytest.mark.gpu
def test_gpu_refused_batches_are_per_batch_results(gpu_engine, oracle_lib):
    check_refusals(gpu_engine, oracle_lib)


@pytest.mark.gpu
def test_gpu_synchronous_errors(gpu_engine):
    check_synchronous_errors(gpu_engine)


# ------------------------------------------------------------------------------------------ 2b. a failed enqueue

def send(gpu, form, msgs, tick, max_rounds):
    if form == "submit":
        gpu.submit(msgs, tick=tick)
    elif form == "submit_raw":
        gpu.submit_raw(msgs, tick=tick, max_rounds=max_rounds)
    else:
        fill_and_commit(gpu, msgs, tick, max_rounds)


def check_failed_enqueue(engine, O, form, flags, groups=24, n_members=3, seed=43):
    """The batch's message copy -- its first stream operation -- fails (the emulation's emu_fail_hip_copy; a device is
    never made to fail): the submitting call returns RGB_E_HIP with the injected code in rgb_last_hip_error, the batch
    is published as failed (collect reports RGB_E_HIP once, then the ring is empty), nothing was applied, and the
    ticket was honoured: the next batches on the same servers, through the same form and through another one, take
    their turn and equal the checker's."""
    import ctypes
    L = engine.lib()
    L.emu_fail_hip_copy.restype, L.emu_fail_hip_copy.argtypes = ctypes.c_int, [ctypes.c_int]
    rng = np.random.default_rng(seed)
    st = fuzz.random_states(rng, groups, n_members, max_runs=6)
    cpu = O.Oracle(groups, n_members, max_runs=16)
    cpu.set_state(0, st)
    R = 3
    other = "submit_raw" if form == "submit" else "submit"

    def good_batch(gpu, via, tick, tag):
        good = multi_round_batch(rng, cpu.get_state(), n_members, 2)
        do, ro = cpu.step(good)
        send(gpu, via, good, tick, R)
        dg, rg, t = gpu.collect()
        assert t == tick and dg.tobytes() == do.tobytes(), tag + ": decisions"
        assert fuzz.sort_rpcs(rg.copy()).tobytes() == fuzz.sort_rpcs(ro).tobytes(), tag + ": rpcs"
        assert_state_equal(tag, gpu.get_state(), cpu.get_state())

    with engine.RaGpuBatch(groups, n_members, ring_capacity=1024, ring_slots=2, max_runs=16, flags=flags) as gpu:
        gpu.set_state(0, st)
        good_batch(gpu, form, 1, "in front of the failed batch")
        lost = multi_round_batch(rng, cpu.get_state(), n_members, 2)       # the checker never sees it
        before_sum, before = gpu.state_checksum(), gpu.get_state()
        injected = L.emu_fail_hip_copy(1)                                  # the next copy: the batch's messages
        try:
            with pytest.raises(engine.RgbError) as e:
                send(gpu, form, lost, 2, R)
        finally:
            L.emu_fail_hip_copy(0)
        assert injected != 0 and (e.value.code, e.value.hip) == (abi.E_HIP, injected), (e.value.code, e.value.hip)
        assert gpu._L.rgb_last_hip_error(gpu._h) == injected
        expect_error(engine, gpu.collect, abi.E_HIP)                       # .. exactly once: the ring moved on
        expect_error(engine, gpu.collect, abi.E_EMPTY)
        assert gpu.in_flight == 0
        assert gpu.state_checksum() == before_sum, "the failed batch changed the state checksum"
        assert_state_equal("the failed batch applied something", gpu.get_state(), before)
        good_batch(gpu, form, 3, f"{form} behind the failed batch")
        good_batch(gpu, other, 4, f"{other} behind the failed batch")
    cpu.close()


@pytest.mark.parametrize("flags", [0, abi.CFG_SUBMIT_TRAINS])
@pytest.mark.parametrize("form", ["submit", "submit_raw", "begin_commit"])
def test_failed_enqueue_is_published_and_honours_its_ticket(emulated_engine, oracle_lib, form, flags):
    """In a worker thread joined with a timeout: a ticket that is not honoured blocks every later submit for ever, and
    that must fail this test, not hang the run."""
    errs = []

    def run():
        try:
            check_failed_enqueue(emulated_engine, oracle_lib, form, flags)
        except BaseException as e:                                   # noqa: BLE001
            errs.append(e)

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(60)
    assert not t.is_alive(), "a submit behind the failed batch never got its turn"
    if errs:
        raise errs[0]


# ------------------------------------------------------------------------------------------ 3. ordering

def check_ordering(engine, O, G=48, N=5, P=4, per=6, seed=57):
    """P threads interleave begin / fill / commit and plain rgb_submit on ONE context, all over the SAME servers: the
    batches come out in the order their slots were taken (noted under a lock around the call that takes the slot), and
    every one equals the checker run in that order."""
    rng = np.random.default_rng(seed)
    st = fuzz.random_states(rng, G, N, max_runs=6)
    batches = {1000 * k + b: multi_round_batch(rng, st, N, 2, frac=0.5) for k in range(P) for b in range(per)}
    total = P * per
    with engine.RaGpuBatch(G, N, ring_capacity=2048, ring_slots=3, max_runs=16) as gpu:
        gpu.set_state(0, st)
        order, got, errs = [], [], []
        take = threading.Lock()

        def producer(k):
            try:
                for b in range(per):
                    tick = 1000 * k + b
                    msgs = batches[tick]
                    while True:
                        try:
                            if (k + b) % 2:
                                with take:                          # rgb_submit takes its slot inside the call
                                    gpu.submit(msgs, tick=tick)
                                    order.append(tick)
                            else:
                                with take:
                                    buf, slot = gpu.submit_begin(2)
                                    order.append(tick)
                                buf[:len(msgs)] = msgs              # filled outside the lock, beside the other producers
                                gpu.submit_commit(slot, len(msgs), tick)
                            break
                        except engine.RgbError as e:
                            if e.code != abi.E_FULL:
                                raise
            except Exception as e:                                   # noqa: BLE001
                errs.append(e)

        def consumer():
            try:
                while len(got) < total and not errs:
                    try:
                        d, r, tick = gpu.collect()
                    except engine.RgbError as e:
                        if e.code != abi.E_EMPTY:
                            raise
                        gpu.wait(20)
                        continue
                    got.append((tick, d.copy(), r.copy()))
            except Exception as e:                                   # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=producer, args=(k,)) for k in range(P)] + [threading.Thread(target=consumer)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not errs, errs
        assert [t for t, _, _ in got] == order, "batches did not come out in the order their slots were taken"
        cpu = O.Oracle(G, N, max_runs=16)
        cpu.set_state(0, st)
        for tick, d, r in got:
            do, ro = cpu.step(batches[tick])
            assert d.tobytes() == do.tobytes(), f"batch {tick}: decisions"
            assert fuzz.sort_rpcs(r).tobytes() == fuzz.sort_rpcs(ro).tobytes(), f"batch {tick}: rpcs"
        assert_state_equal("final", gpu.get_state(), cpu.get_state())
        cpu.close()


def test_interleaved_begin_commit_and_submit_keep_slot_order(emulated_engine, oracle_lib):
    check_ordering(emulated_engine, oracle_lib)


@pytest.mark.gpu
def test_gpu_interleaved_begin_commit_and_submit_keep_slot_order(gpu_engine, oracle_lib):
    check_ordering(gpu_engine, oracle_lib, G=256, per=8)


# ------------------------------------------------------------------------------------------ 4. the trains fall-back

def check_trains_fallback(engine, O, G=1200, N=5):
    """On a context opened with RGB_CFG_SUBMIT_TRAINS the raw calls run rgb_submit's host passes: the same results as
    rgb_submit (a big multi-round batch still runs as a train), the same per-batch errors."""
    rng = np.random.default_rng(99)
    st = fuzz.random_states(rng, G, N, max_runs=6)
    cpu = O.Oracle(G, N, max_runs=16)
    cpu.set_state(0, st)
    mk = lambda: engine.RaGpuBatch(G, N, ring_capacity=65536, ring_slots=2, max_runs=16, flags=abi.CFG_SUBMIT_TRAINS)
    with mk() as a, mk() as b:
        a.set_state(0, st)
        b.set_state(0, st)
        for k in range(2):
            msgs = multi_round_batch(rng, cpu.get_state(), N, 4, frac=0.9)
            msgs = msgs[msgs["kind"] != abi.MSG_NOP]
            assert len(msgs) >= 4096
            do, ro = cpu.step(msgs)
            a.submit(msgs, tick=k)
            da, ra, _ = a.collect()
            if k:
                b.submit_raw(msgs, tick=k, max_rounds=4)
            else:
                fill_and_commit(b, msgs, k, 4)
            db, rb, tick = b.collect()
            assert tick == k and db.tobytes() == da.tobytes() and rb.tobytes() == ra.tobytes()
            assert db.tobytes() == do.tobytes()
            assert fuzz.sort_rpcs(rb).tobytes() == fuzz.sort_rpcs(ro).tobytes()
            assert_state_equal(f"batch {k}", b.get_state(), cpu.get_state())
        assert b.submit_trains() == a.submit_trains() == 2
    cpu.close()
    check_refusals(engine, O, flags=abi.CFG_SUBMIT_TRAINS)
    check_synchronous_errors(engine, flags=abi.CFG_SUBMIT_TRAINS)


def test_trains_fallback_on_the_emulation(emulated_engine, oracle_lib):
    check_trains_fallback(emulated_engine, oracle_lib)


def test_trains_fallback_sees_an_invalid_record_behind_65536_messages_of_one_server(emulated_engine):
    """rgb_submit's pass over the batch stops at a server's 65 536th message; the raw call still reports the invalid
    record behind it (RGB_E_INVAL before RGB_E_UNSUPPORTED), and RGB_E_UNSUPPORTED when there is none."""
    engine = emulated_engine
    with engine.RaGpuBatch(8, 3, ring_capacity=65540, ring_slots=1, flags=abi.CFG_SUBMIT_TRAINS) as gpu:
        batch = np.zeros(65537, dtype=abi.MSG_DTYPE)
        batch["server"], batch["kind"] = 5, abi.MSG_PIPELINE_RPCS
        before = gpu.state_checksum()
        for last, code in ((batch[0], abi.E_UNSUPPORTED), (dict((n, r) for n, r, _ in bad_records(24))["aer_run0"], abi.E_INVAL)):
            batch[-1] = last
            gpu.submit_raw(batch, max_rounds=1)
            expect_error(engine, gpu.collect, code)
            expect_error(engine, gpu.collect, abi.E_EMPTY)
            assert gpu.state_checksum() == before


@pytest.mark.gpu
def test_gpu_trains_fallback(gpu_engine, oracle_lib):
    check_trains_fallback(gpu_engine, oracle_lib, G=1500)


# ------------------------------------------------------------------------------------------ 4b. spread batches

SPREAD_N, SPREAD_ROUNDS = 5, 8
SPREAD_GROUPS = 52              # the fewest groups of five with groups x n_members >= 256: a tick spans two workgroups
SPREAD_LAYOUTS = ("round-major", "server-major", "round-major reversed", "server-major reversed")


def spread_batch(rng, state, n_members, rounds, layout):
    """`rounds` ticks with a message for EVERY server (frac = 1.0), laid out on purpose instead of shuffled:
    round-major   the ticks one behind the other, each in server order: a server's messages lie exactly len(state)
                  records apart, each in another workgroup of 256 records
    server-major  a stable sort of that by server: a server's messages are adjacent, inside one wavefront
    `... reversed`: the same records back to front."""
    ticks = [fuzz.random_msgs(rng, state, n_members, frac=1.0) for _ in range(rounds)]
    msgs = np.concatenate([t[np.argsort(t["server"], kind="stable")] for t in ticks])
    assert len(msgs) == rounds * len(state)
    if layout.startswith("server-major"):
        msgs = msgs[np.argsort(msgs["server"], kind="stable")]
    if layout.endswith("reversed"):
        msgs = msgs[::-1].copy()
    return msgs


def check_spread_batches(engine, O, groups, n_members=SPREAD_N, rounds=SPREAD_ROUNDS, seed=71, tag=""):
    """Every layout of SPREAD_LAYOUTS through rgb_submit (A), rgb_submit_raw (B) and begin / commit (C): decisions and
    rpc records byte-equal between the three and equal to the sequential checker's, the states as check_differential
    compares them."""
    rng = np.random.default_rng(seed)
    S = groups * n_members
    assert S >= 256
    st = fuzz.random_states(rng, groups, n_members, max_runs=6)
    cpu = O.Oracle(groups, n_members, max_runs=16)
    cpu.set_state(0, st)
    n = rounds * S
    ring_capacity = sum(n // (r + 1) for r in range(rounds))
    mk = lambda: engine.RaGpuBatch(groups, n_members, ring_capacity=ring_capacity, ring_slots=2, max_runs=16)
    with mk() as a, mk() as b, mk() as c:
        for g in (a, b, c):
            g.set_state(0, st)
        assert b.raw_capacity(rounds) >= n
        for k, layout in enumerate(SPREAD_LAYOUTS):
            msgs = spread_batch(rng, cpu.get_state(), n_members, rounds, layout)
            where = f"{tag}{layout}, {groups} groups of {n_members}, {len(msgs)} messages"
            # the layout is what it says: a server's messages a tick apart, or adjacent
            live = np.flatnonzero(msgs["server"] == msgs["server"][0])
            assert len(live) == rounds, where
            if layout.startswith("round-major"):
                assert np.all(np.diff(live) == S) and len(set(live // 256)) == rounds, where
            else:
                assert np.all(np.diff(live) == 1), where
            do, ro = cpu.step(msgs)
            a.submit(msgs, tick=k)
            da, ra, _ = a.collect()
            b.submit_raw(msgs, tick=k, max_rounds=rounds)
            db, rb, tb = b.collect()
            fill_and_commit(c, msgs, k, rounds)
            dc, rc, tc, slot = c.collect_view()
            assert tb == k and tc == k, where
            assert db.tobytes() == da.tobytes(), where + ": raw decisions differ from rgb_submit's"
            assert rb.tobytes() == ra.tobytes(), where + ": raw rpc records differ from rgb_submit's"
            assert dc.tobytes() == da.tobytes() and rc.tobytes() == ra.tobytes(), where + ": begin/commit + view"
            c.release(slot)
            assert db.tobytes() == do.tobytes(), where + ": decisions differ from the checker's"
            assert fuzz.sort_rpcs(rb.copy()).tobytes() == fuzz.sort_rpcs(ro).tobytes(), where + ": rpcs vs checker"
            want = cpu.get_state()
            assert_state_equal(where + " (rgb_submit)", a.get_state(), want)
            assert_state_equal(where + " (rgb_submit_raw)", b.get_state(), want)
            assert_state_equal(where + " (begin/commit)", c.get_state(), want)
    cpu.close()


@pytest.mark.parametrize("sched", ("ascending",) + PERMUTED_SCHEDULES)
def test_spread_batches(emulated_engine, oracle_lib, sched):
    with schedule(emulated_engine, sched) as tag:
        check_spread_batches(emulated_engine, oracle_lib, SPREAD_GROUPS, tag=tag + ": ")


@pytest.mark.gpu
def test_gpu_spread_batches(gpu_engine, oracle_lib):
    check_spread_batches(gpu_engine, oracle_lib, SPREAD_GROUPS * 16)


# ------------------------------------------------------------------------------------------ 4c. permuted schedules

@pytest.mark.parametrize("sched", PERMUTED_SCHEDULES)
def test_raw_path_under_permuted_schedules(emulated_engine, oracle_lib, sched):
    """The emulation runs workgroups and lanes in index order unless told otherwise, and then every atomic of
    rgb_prepare.hip arrives in submission order: its sorting step has nothing to do.  The checks of this module once
    more with the workgroups and the lanes reversed, and permuted (tests/emu_schedule.py); the referee stays the
    sequential checker.  check_trains_fallback runs with 260 groups, the fewest whose batches stay above its own floor
    of 4096 messages with some room (at the 1200 of test_trains_fallback_on_the_emulation it alone costs more than the
    rest of this module): on such a context the raw calls run rgb_submit's host passes and launch no kernel of
    rgb_prepare.hip; what the schedules reach there is the train launch of rgb_submit, on the emulation always the
    persistent form (see test_train_on_the_block_emulation_under_permuted_schedules)."""
    with schedule(emulated_engine, sched):
        for n_members, rounds, groups, seed in DIFF_CASES:
            try:
                check_differential(emulated_engine, oracle_lib, n_members, rounds, groups, seed)
            except AssertionError as e:
                raise AssertionError(f"DIFF_CASES N={n_members} rounds={rounds} seed={seed}: {e}") from e
        check_refusals(emulated_engine, oracle_lib)
        check_ordering(emulated_engine, oracle_lib)
        check_trains_fallback(emulated_engine, oracle_lib, G=260)


# ------------------------------------------------------------------------------------------ 5. resources

def test_prepare_kernels_use_no_scratch():
    """hipcc's resource remarks for gfx950 (no GPU needed), as tests/test_kernel_resources.py reads them: every kernel
    of rgb_prepare.hip without scratch or spills, a few KiB of LDS, full occupancy."""
    from test_kernel_resources import HIPCC, _parse
    if HIPCC is None:
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "ra_amd", "csrc", "rgb_prepare.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-mllvm",
                        "-disable-machine-licm", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage = _parse(r.stderr)
    names = [k for k in usage if "rgb_prep_" in k]
    assert len(names) == 3, names                       # scan, rounds, scatter
    for k in names:
        u = usage[k]
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, f"{k}: {u}"
        assert u["Occupancy"] >= 8 and u["LDS Size"] <= 4096 and u["VGPRs"] <= 64, f"{k}: {u}"


# ------------------------------------------------------------------------------------------ 6. GPU sizes

@pytest.mark.gpu
def test_gpu_closed_loop_65536x5_through_the_raw_path(gpu_engine, oracle_lib):
    """The closed-loop workload at the benchmark's size (65 536 groups of five; the host generator gives ~129 k messages
    per tick, 177 k .. 95 k over these ticks) submitted through the raw path, every tick as two batches in flight at once
    -- its halves, 3 MiB and more each, so every copy takes the copy stream --, every decision and rpc record against the checker; then
    a two-round 131 072-message batch (8 MiB) and the whole final state."""
    from ra_amd import workload as W
    G, N, seed, ticks = 65536, 5, 0x5EED0003, 4
    st = W.initial_states(G, N, seed)
    cpu = oracle_lib.Oracle(G, N, max_runs=16)
    cpu.set_state(0, st)
    with gpu_engine.RaGpuBatch(G, N, max_runs=16, ring_capacity=262144, ring_slots=3) as gpu:
        gpu.set_state(0, st)
        assert gpu.raw_capacity(1) == 262144 and gpu.raw_capacity(2) >= 131072
        n_dec = 0
        for t in range(ticks):
            m = W.gen_tick(cpu.get_state(), N, t, seed, W.MIX_CONFIG3)
            HALF = len(m) // 2
            assert HALF * 64 >= 2 << 20                           # both halves are copy-stream sized
            do, ro = cpu.step(m)
            # two batches in flight at once: the second's copy runs under the first's kernels
            gpu.submit_raw(m[:HALF], tick=2 * t, max_rounds=1)
            fill_and_commit(gpu, m[HALF:], 2 * t + 1, 1)
            d0, r0, t0 = gpu.collect()
            d1, r1, t1 = gpu.collect()
            assert (t0, t1) == (2 * t, 2 * t + 1)
            dg = np.concatenate([d0, d1])
            r1 = r1.copy()
            r1["msg_index"] += HALF
            rg = np.concatenate([r0, r1])
            if dg.tobytes() != do.tobytes():
                bad = int(np.flatnonzero((dg.view(np.uint8).reshape(-1, 64) != do.view(np.uint8).reshape(-1, 64)).any(axis=1))[0])
                raise AssertionError(f"tick {t} slot {bad}: msg={m[bad]}\n gpu={dg[bad]}\n cpu={do[bad]}")
            assert fuzz.sort_rpcs(rg).tobytes() == fuzz.sort_rpcs(ro).tobytes(), f"tick {t}: rpcs differ"
            n_dec += len(m)
        assert n_dec > ticks * 65536
        # 131 072 messages in two rounds: the head of a tick, then the head of the next tick (mostly the same servers)
        ma = W.gen_tick(cpu.get_state(), N, ticks, seed, W.MIX_CONFIG3)[:65536]
        do_a, ro_a = cpu.step(ma)
        mb = W.gen_tick(cpu.get_state(), N, ticks + 1, seed, W.MIX_CONFIG3)[:65536]
        assert len(ma) + len(mb) == 131072 and np.isin(mb["server"], ma["server"]).sum() > 16384
        do_b, ro_b = cpu.step(mb)
        both = np.concatenate([ma, mb])
        dg, rg = gpu.step_raw(both, max_rounds=2)
        assert dg.tobytes() == np.concatenate([do_a, do_b]).tobytes(), "two-round 131 072-message batch: decisions"
        ro_b = ro_b.copy()
        ro_b["msg_index"] += len(ma)
        assert fuzz.sort_rpcs(rg).tobytes() == fuzz.sort_rpcs(np.concatenate([ro_a, ro_b])).tobytes()
        assert_state_equal("final", gpu.get_state(), cpu.get_state())
    cpu.close()
