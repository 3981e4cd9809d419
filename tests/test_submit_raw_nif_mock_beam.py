"""submit_raw/4 of the Erlang NIF shim (ra_amd/csrc/ra_gpu_batch_nif.c) EXECUTED on the mock BEAM of
tests/test_nif_shim_mock_beam.py, on top of the CPU-emulated library: the same batch fans back to the owning processes
exactly as through submit/3, and a batch the device refuses reaches the owners the way a batch whose enqueue failed
does -- {error, _} once from collect/1, {ra_gpu_batch_error, _} to the default owner from the collector thread."""
import numpy as np

import fuzz
import test_nif_shim_mock_beam as M
from ra_amd import abi

beam = M.beam              # the module-scoped fixture: the shim + the mock linked against the emulated library
Opaque = M.Opaque


def _open(beam, G, N, st, slots=4, cap=2048):
    ok, ctx = beam.call("open", 0, 16, slots, cap)
    assert ok == "ok"
    assert beam.call("register_groups", ctx, G, N) == "ok"
    assert beam.call("upload_state", ctx, 0, st.tobytes()) == "ok"
    return ctx


def _two_rounds(rng, state, N):
    msgs = np.concatenate([fuzz.random_msgs(rng, state, N, frac=0.7) for _ in range(2)])
    rng.shuffle(msgs)
    return msgs


def test_submit_raw_round_trip_and_arguments(beam, oracle_lib):
    G, N = 48, 5
    rng = np.random.default_rng(177)
    st = fuzz.random_states(rng, G, N, max_runs=6)
    cpu = oracle_lib.Oracle(G, N, max_runs=16)
    cpu.set_state(0, st)
    ctx = _open(beam, G, N, st)
    assert beam.call("submit_raw", ctx, b"\0" * 63, 1, 4) == "badarg"
    assert beam.call("submit_raw", 17, b"", 1, 4) == "badarg"
    assert beam.call("submit_raw", ctx, b"", 1, "four") == "badarg"
    assert beam.call("submit_raw", ctx, b"", 1, 9) == ("error", "invalid")              # max_rounds above 8
    assert beam.L.mock_func_flags(b"submit_raw", 4) == 2                                # dirty IO-bound: it may wait
    for tick in range(1, 4):
        msgs = _two_rounds(rng, cpu.get_state(), N)
        want_d, want_r = cpu.step(msgs)
        assert beam.call("submit_raw", ctx, msgs.tobytes(), tick, 2) == "ok"
        ok, got_tick, n, dec_bin, rpc_bin = beam.call("collect", ctx)
        assert (ok, got_tick, n) == ("ok", tick, len(msgs))
        assert dec_bin == want_d.tobytes(), f"tick {tick}: decisions differ"
        got_r = np.frombuffer(rpc_bin, dtype=abi.RPC_DTYPE)
        assert fuzz.sort_rpcs(got_r.copy()).tobytes() == fuzz.sort_rpcs(want_r).tobytes(), f"tick {tick}: rpcs"
    # a refused batch through collect/1: the error once, then the ring is empty and the next batch runs
    bad = _two_rounds(rng, cpu.get_state(), N)
    bad["server"][len(bad) // 2] = G * N
    bad["kind"][len(bad) // 2] = abi.MSG_AER
    assert beam.call("submit_raw", ctx, bad.tobytes(), 50, 2) == "ok"                   # nothing is checked in the call
    assert beam.call("collect", ctx) == ("error", "invalid")
    assert beam.call("collect", ctx) == ("error", "empty")
    three = np.zeros(3, dtype=abi.MSG_DTYPE)
    three["server"], three["kind"] = 7, abi.MSG_PIPELINE_RPCS
    assert beam.call("submit_raw", ctx, three.tobytes(), 51, 2) == "ok"
    assert beam.call("collect", ctx) == ("error", "unsupported")
    ok, state_bin = beam.call("download_state", ctx, 0, G * N)
    assert ok == "ok" and state_bin == cpu.get_state().tobytes(), "a refused batch applied something"
    msgs = _two_rounds(rng, cpu.get_state(), N)
    want_d, _ = cpu.step(msgs)
    assert beam.call("submit_raw", ctx, msgs.tobytes(), 52, 2) == "ok"
    ok, got_tick, n, dec_bin, _ = beam.call("collect", ctx)
    assert (ok, got_tick, dec_bin) == ("ok", 52, want_d.tobytes())
    beam.L.mock_gc_resource_term(ctx.t)
    cpu.close()


def test_submit_raw_fans_back_like_submit(beam, oracle_lib):
    """Two contexts from one state, one owner process per group on both: the same batch through submit/3 on the one
    and submit_raw/4 on the other gives every owner the same message; then a refused batch ends the collector with
    {ra_gpu_batch_error, {error, invalid}} to the default owner, as a failed batch does."""
    G, N = 40, 5
    rng = np.random.default_rng(179)
    st = fuzz.random_states(rng, G, N, max_runs=6)
    cpu = oracle_lib.Oracle(G, N, max_runs=16)
    cpu.set_state(0, st)
    ctxs = [_open(beam, G, N, st), _open(beam, G, N, st)]
    for ctx in ctxs:
        for g in range(30):
            assert beam.call("register_owner", ctx, g * N, N, Opaque(beam.L.mock_pid(1000 + g))) == "ok"
        assert beam.call("start_collector", ctx, Opaque(beam.L.mock_pid(4242))) == "ok"
    owner_of = lambda srv: 1000 + srv // N if srv // N < 30 else 4242
    for tick in range(1, 4):
        msgs = _two_rounds(rng, cpu.get_state(), N)
        want_d, _ = cpu.step(msgs)
        owners = sorted({owner_of(int(s)) for s in want_d["server"]})
        got = []
        for k, ctx in enumerate(ctxs):
            if k == 0:
                assert beam.call("submit", ctx, msgs.tobytes(), tick) == "ok"
            else:
                assert beam.call("submit_raw", ctx, msgs.tobytes(), tick, 2) == "ok"
            box = {}
            for _ in owners:
                to, msg = beam.recv()
                assert msg is not None, "an owner got nothing"
                assert msg[0] == "ra_gpu_batch" and msg[1] == tick and to not in box
                box[to] = msg
            assert sorted(box) == owners
            got.append(box)
        assert got[0] == got[1], f"tick {tick}: submit_raw/4 fanned back something else than submit/3"
        for o in owners:
            idx = [i for i, d in enumerate(want_d) if owner_of(int(d["server"])) == o]
            assert got[1][o][3] == want_d[idx].tobytes(), f"owner {o}: decisions"
    assert beam.recv(timeout_ms=200) == (None, None)
    bad = _two_rounds(rng, cpu.get_state(), N)
    bad["kind"][0] = abi.MSG_TRANSFER_LEADERSHIP + 1
    assert beam.call("submit_raw", ctxs[1], bad.tobytes(), 9, 2) == "ok"
    to, msg = beam.recv()
    assert to == 4242 and msg == ("ra_gpu_batch_error", ("error", "invalid"))
    assert beam.recv(timeout_ms=200) == (None, None)
    ok, state_bin = beam.call("download_state", ctxs[1], 0, G * N)
    assert ok == "ok" and state_bin == cpu.get_state().tobytes()
    # the thread ended by itself (as after a failed batch): a new collector may be started, and the ring moved on
    assert beam.call("start_collector", ctxs[1], Opaque(beam.L.mock_pid(4242))) == "ok"
    msgs = _two_rounds(rng, cpu.get_state(), N)
    want_d, _ = cpu.step(msgs)
    assert beam.call("submit_raw", ctxs[1], msgs.tobytes(), 10, 2) == "ok"
    n_owners = len({owner_of(int(s)) for s in want_d["server"]})
    total = 0
    for _ in range(n_owners):
        to, msg = beam.recv()
        assert msg is not None and msg[0] == "ra_gpu_batch" and msg[1] == 10
        total += msg[2]
    assert total == len(msgs)
    for ctx in ctxs:
        assert beam.call("stop_collector", ctx) == "ok"
        beam.L.mock_gc_resource_term(ctx.t)
    cpu.close()
