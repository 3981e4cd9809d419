"""{transfer_leadership, Target} on the device (ABI v10): the leader's clause of src/ra_server.erl:996-1035, the other
roles' unsupported_call reply, and the leader's await condition transfer_leadership_condition/2 (:2235-2245,
handle_await_condition/2 :1916-1959).

* the hand-transcribed vectors of tests/golden/transfer_leadership_vectors.json (test/ra_server_SUITE.erl:1096-1133
  plus source-derived vectors for the condition), through the engine;
* the boundary: reason 5 round-trips through upload / download and 6 is refused, kind 16 is accepted and 17 refused;
* the same answer on every path: ticks that mix transfers (and servers awaiting one) into the ordinary random mix
  give byte-identical decisions and state through rgb_submit / rgb_collect, rgb_run_ticks_device with and without
  kind counts, and a train launch -- and those are the decisions and the state of the sequential CPU checker.

Each test runs on the CPU emulation of the HIP sources (emulated_engine) and, under -m gpu, on the MI355X."""
import json
import os

import numpy as np
import pytest

from ra_amd import abi
from ra_amd import effects as fx
import fuzz
from test_train import Buf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transfer_leadership_vectors.json")
ROLE = {"follower": abi.ROLE_FOLLOWER, "candidate": abi.ROLE_CANDIDATE, "leader": abi.ROLE_LEADER,
        "pre_vote": abi.ROLE_PRE_VOTE, "await_condition": abi.ROLE_AWAIT_CONDITION}
COND = {"none": abi.COND_NONE, "transfer_leadership": abi.COND_TRANSFER_LEADERSHIP}


def load_vectors():
    with open(GOLDEN) as f:
        return json.load(f)["vectors"]


def slot(name):
    return abi.NONE if name is None else int(name[1:]) - 1


def base_state(v):
    """base_state(3, _) (test/ra_server_SUITE.erl:4151-4192) in row 0 of a one-group state, with the vector's tweaks."""
    n = 3
    st = abi.empty_server_states(1, n)
    st["current_term"][0] = 5
    st["commit_index"][0] = 3
    st["last_applied"][0] = 3
    st["leader_id"][0] = 0
    abi.set_log(st, 0, [(0, 0), (1, 1), (2, 3), (3, 5)], last_written=(3, 5))
    st["next_index"][0, :n] = 4
    st["match_index"][0, :n] = 3
    st["role"][0] = ROLE[v["role"]]
    st["cond_reason"][0] = COND[v.get("cond_reason", "none")]
    tw = v.get("tweak") or {}
    if "non_voter" in tw:
        st["voter_mask"][0] = int(st["voter_mask"][0]) & ~(1 << slot(tw["non_voter"])) & 0xFF
    for name, peer in (tw.get("peer") or {}).items():
        for k, val in peer.items():
            st[k][0, slot(name)] = val
    return st


def vector_msg(v):
    m = v["msg"]
    kind = m.get("kind", "transfer_leadership")
    if kind == "transfer_leadership":
        rec = fx.TransferLeadership(None if m["target"] is None else slot(m["target"]))
    elif kind == "aer":
        rec = fx.AppendEntriesRpc(m["term"], slot(m["from"]), m["commit"], m["prev"][0], m["prev"][1])
    elif kind == "heartbeat_rpc":
        rec = fx.HeartbeatRpc(m["query_index"], m["term"], slot(m["from"]))
    elif kind == "request_vote_rpc":
        rec = fx.RequestVoteRpc(m["term"], slot(m["from"]), m["last"][0], m["last"][1])
    elif kind == "election_timeout":
        rec = fx.ElectionTimeout(m["token"])
    else:
        assert kind == "await_condition_timeout", kind
        rec = fx.AWAIT_CONDITION_TIMEOUT
    return np.array([fx.encode(0, rec)], dtype=abi.MSG_DTYPE)


def as_effect(e):
    """A JSON effect of the vectors as ra_amd.effects.decode spells it (member names -> slots in send_msg)."""
    if isinstance(e, list):
        t = tuple(as_effect(x) for x in e)
        return (t[0], slot(t[1])) + t[2:] if t and t[0] == "send_msg" else t
    return e


def run_vectors(eng):
    seen = []
    for v in load_vectors():
        st0 = base_state(v)
        eng.set_state(0, st0)
        msg = vector_msg(v)
        dec, rpcs = eng.step(msg)
        row0, row1 = st0[0], eng.get_state()[0]
        d, ex, tag = dec[0], v["expect"], f'{v["id"]} ({v["source"]}): {v["what"]}'
        fl = int(d["flags"])
        assert not fl & (abi.F_INVARIANT | abi.F_UNHANDLED), (tag, hex(fl))
        assert int(d["role"]) == ROLE[ex["role"]] == int(row1["role"]), (tag, int(d["role"]), int(row1["role"]))
        if ex.get("state_unchanged"):
            assert row1.tobytes() == row0.tobytes(), tag
        if "cond_reason" in ex:
            assert int(row1["cond_reason"]) == COND[ex["cond_reason"]], tag
        for k, val in (ex.get("state") or {}).items():
            want = slot(val) if k in ("leader_id", "voted_for") else val
            assert int(row1[k]) == want, (tag, k, int(row1[k]), want)
        assert bool(fl & abi.F_REPROCESSED) == bool(ex.get("reprocessed")), (tag, hex(fl))
        effects = fx.decode(msg[0], d, rpcs, row1, 3)
        if "effects" in ex:
            assert effects == [as_effect(e) for e in ex["effects"]], (tag, effects)
        if "reply" in ex:
            r = ex["reply"]
            want = ("cast", slot(r["to"]), (0, fx.AppendEntriesReply(r["term"], r["success"], r["next_index"],
                                                                      r["last_index"], r["last_term"])))
            assert want in effects, (tag, effects)
        if "vote" in ex:
            assert ("reply", fx.RequestVoteResult(ex["vote"]["term"], ex["vote"]["granted"])) in effects, (tag, effects)
        if "pre_vote_requests" in ex:
            p = ex["pre_vote_requests"]
            reqs = [e for e in effects if e[0] == "send_vote_requests"]
            assert len(reqs) == 1 and [s for s, _ in reqs[0][1]] == [1, 2], (tag, effects)
            for _, rec in reqs[0][1]:
                assert isinstance(rec, fx.PreVoteRpc) and (rec.term, rec.last_log_index, rec.last_log_term) == (
                    p["term"], p["last_index"], p["last_term"]) and rec.candidate_id == 0, (tag, rec)
        seen.append(v["id"])
    assert seen == ["T1", "T2", "T3", "T4", "T5", "C1", "C2", "C3", "C4", "C5", "C6"]


def test_vector_file_cites_the_reference():
    vs = load_vectors()
    assert all(v["source"].startswith(("test/ra_server_SUITE.erl:", "src/ra_server.erl:")) for v in vs)
    assert sum(v["source"].startswith("test/ra_server_SUITE.erl:") for v in vs) == 5


def test_reference_vectors_on_the_emulated_engine(emulated_engine):
    with emulated_engine.RaGpuBatch(1, 3, ring_capacity=16, ring_slots=2, max_runs=16) as eng:
        run_vectors(eng)


@pytest.mark.gpu
def test_reference_vectors_on_the_gpu():
    from ra_amd import engine
    with engine.RaGpuBatch(1, 3, ring_capacity=16, ring_slots=2, max_runs=16) as eng:
        run_vectors(eng)


# ---------------------------------------------------------------------------------------------------- the boundary
def check_abi(engine):
    L = engine.lib()
    assert L.rgb_abi_version() == abi.ABI_VERSION == 10
    assert abi.N_KINDS == abi.MSG_TRANSFER_LEADERSHIP + 1 == 17 and abi.KIND_RANK[abi.MSG_TRANSFER_LEADERSHIP] == 14
    G, N = 4, 3
    with engine.RaGpuBatch(G, N, ring_capacity=64, ring_slots=2, max_runs=16) as eng:
        st = abi.empty_server_states(G, N)
        st["role"][0] = abi.ROLE_AWAIT_CONDITION
        st["cond_reason"][0] = abi.COND_TRANSFER_LEADERSHIP
        st["role"][1] = abi.ROLE_AWAIT_CONDITION
        st["cond_reason"][1] = abi.COND_WAL_DOWN_LEADER
        st["role"][2] = abi.ROLE_AWAIT_CONDITION
        st["cond_reason"][2] = abi.COND_MISSING
        eng.set_state(0, st)
        assert eng.get_state().tobytes() == st.tobytes()               # reason 5 comes back unchanged
        # the checksum tells the reasons apart (the condition field is two bits and a flag on the device)
        sums = set()
        for reason in (abi.COND_MISSING, abi.COND_WAL_DOWN_LEADER, abi.COND_TRANSFER_LEADERSHIP):
            one = st.copy()
            one["cond_reason"][0] = reason
            eng.set_state(0, one)
            sums.add(eng.state_checksum(0, 1))
        assert len(sums) == 3
        eng.set_state(0, st)
        bad = st.copy()
        bad["cond_reason"][3] = abi.COND_TRANSFER_LEADERSHIP + 1
        with pytest.raises(engine.RgbError):
            eng.set_state(0, bad)
        assert eng.get_state().tobytes() == st.tobytes()               # refused as a whole: nothing was uploaded
        m = np.array([fx.encode(4, fx.TransferLeadership(1))], dtype=abi.MSG_DTYPE)
        dec, _ = eng.step(m)                                           # kind 16 is accepted (a follower: unsupported)
        assert int(dec["flags"][0]) == abi.F_CALL_REPLY and int(dec["reply_next_index"][0]) == abi.CALL_UNSUPPORTED
        m["kind"] = abi.MSG_TRANSFER_LEADERSHIP + 1
        with pytest.raises(engine.RgbError):
            eng.submit(m)


def test_abi_v10_on_the_emulated_engine(emulated_engine):
    check_abi(emulated_engine)


@pytest.mark.gpu
def test_abi_v10_on_the_gpu():
    from ra_amd import engine
    check_abi(engine)


def test_effects_encode_and_decode_the_call():
    m = fx.encode(7, fx.TransferLeadership(2))
    assert (int(m["kind"]), int(m["from"]), int(m["server"])) == (abi.MSG_TRANSFER_LEADERSHIP, 2, 7)
    assert int(fx.encode(7, fx.TransferLeadership(None))["from"]) == abi.NONE
    raw = np.array([m], dtype=abi.MSG_DTYPE).view(np.uint8)
    assert raw[8:].sum() == 0                                          # no other field is used
    d = np.zeros(1, dtype=abi.DECISION_DTYPE)[0]
    d["flags"], d["reply_to"], d["reply_next_index"] = abi.F_CALL_REPLY | abi.F_ROLE_CHANGED, 2, abi.CALL_OK
    st = abi.empty_server_states(3, 3)[7]
    assert fx.decode(m, d, [], st, 3) == [("reply", "ok"), ("send_msg", 2, "election_timeout", "cast")]
    d["reply_to"] = abi.NONE
    for code, want in ((abi.CALL_ALREADY_LEADER, "already_leader"), (abi.CALL_UNKNOWN_MEMBER, ("error", "unknown_member")),
                       (abi.CALL_NON_VOTER, ("error", "non_voter")), (abi.CALL_NOT_UP_TO_DATE, ("error", "not_up_to_date")),
                       (abi.CALL_UNSUPPORTED, ("error", ("unsupported_call", ("transfer_leadership", 2))))):
        d["reply_next_index"] = code
        assert fx.decode(m, d, [], st, 3) == [("reply", want)]


# ---------------------------------------------------------------------------------------------- every path
def mixed_ticks_states(rng, G, N):
    """Random states in which some leaders are level with a peer and some servers await a transfer."""
    st = fuzz.random_states(rng, G, N, max_runs=6)
    for s in range(len(st)):
        row = st[s]
        if int(row["role"]) == abi.ROLE_LEADER and rng.random() < 0.6:
            st["next_index"][s, int(rng.integers(0, N))] = ra_log_next_index(row)
        elif int(row["role"]) == abi.ROLE_AWAIT_CONDITION and rng.random() < 0.6:
            st["cond_reason"][s] = abi.COND_TRANSFER_LEADERSHIP
    return st


def ra_log_next_index(row):                                           # src/ra_log.erl:1166-1174
    if int(row["first_index"]) <= int(row["last_index"]):
        return int(row["last_index"]) + 1
    if int(row["snapshot_index"]) != abi.UNDEF_INT:
        return int(row["snapshot_index"]) + 1
    return 0


def with_transfers(rng, m, st, N):
    """The ordinary random mix with a quarter of it turned into transfer calls (targets: self, members, slots beyond
    the group, RGB_NONE), NOPs dropped."""
    m = m[m["kind"] != abi.MSG_NOP].copy()
    for q in np.flatnonzero(rng.random(len(m)) < 0.25):
        s = int(m["server"][q])
        lvl = [j for j in range(N) if int(st["next_index"][s, j]) == ra_log_next_index(st[s])]
        choices = [int(st["self"][s]), abi.NONE, min(N, 7)] + lvl * 3 + list(range(N))
        rec = np.zeros(1, dtype=abi.MSG_DTYPE)
        rec["server"], rec["kind"], rec["from"] = s, abi.MSG_TRANSFER_LEADERSHIP, int(rng.choice(choices))
        m[q] = rec[0]
    return m


def check_every_path(engine, oracle_lib, G, N, T, seed, on_gpu):
    from ra_amd import engine as engine_mod
    train_bucket = engine_mod.train_bucket
    rng = np.random.default_rng(seed)
    S = G * N
    eng = engine.RaGpuBatch(G, N, max_runs=16, ring_slots=2, ring_capacity=S)
    st0 = mixed_ticks_states(rng, G, N)
    eng.set_state(0, st0)
    cpu = oracle_lib.Oracle(G, N, max_runs=16)                        # the sequential checker, bounded like the device
    cpu.set_state(0, st0)
    ticks, want_dec, codes = [], [], set()
    for t in range(T):
        st = eng.get_state()
        m = with_transfers(rng, fuzz.random_msgs(rng, st, N), st, N)
        m = m[np.argsort(train_bucket(m["kind"], m["flags"], m["server"], N), kind="stable")]   # bucket order
        dec, _ = eng.step(m)                                           # rgb_submit / rgb_collect: class kernels
        do, _ = cpu.step(m)
        assert dec.tobytes() == do.tobytes(), f"rgb_submit against the checker: tick {t}"
        assert eng.get_state().tobytes() == cpu.get_state().tobytes(), f"state against the checker: tick {t}"
        ticks.append(m)
        want_dec.append(dec)
        tr = dec[m["kind"] == abi.MSG_TRANSFER_LEADERSHIP]
        assert np.all(tr["flags"] & abi.F_CALL_REPLY | (tr["role"] == abi.ROLE_AWAIT_CONDITION))
        codes |= set(int(c) for c in tr["reply_next_index"][(tr["flags"] & abi.F_CALL_REPLY) != 0])
    st_end = eng.get_state()
    cpu.close()
    assert codes == set(range(6)), codes                              # every reply of the call came up
    replay_on_the_device_paths(eng, S, N, st0, ticks, want_dec, st_end, on_gpu)
    eng.close()


def replay_on_the_device_paths(eng, S, N, st0, ticks, want_dec, st_end, on_gpu):
    """Ticks in bucket order (at most one message per server) from st0 through rgb_run_ticks_device with and without
    kind counts and through one train launch: the decisions of every tick must be want_dec, the final state st_end."""
    from ra_amd import engine as engine_mod
    train_bucket = engine_mod.train_bucket
    T = len(ticks)
    tb = S * 64
    msgs = Buf(T * tb, on_gpu)
    host = np.zeros(T * tb, dtype=np.uint8)
    for t, m in enumerate(ticks):
        host[t * tb:t * tb + len(m) * 64] = m.view(np.uint8)
    if on_gpu:
        import torch
        msgs.t.copy_(torch.from_numpy(host))
    else:
        msgs.a[:len(host)] = host
    counts = np.array([len(m) for m in ticks], dtype=np.uint32)
    kinds = np.stack([np.bincount(m["kind"], minlength=abi.N_KINDS)[:abi.N_KINDS] for m in ticks]).astype(np.uint32)

    def compare(dec_buf, what):
        for t in range(T):
            got = abi.expand_decisions(dec_buf.host()[t * tb:t * tb + int(counts[t]) * 64].view(abi.DECISION_DTYPE))
            assert got.tobytes() == want_dec[t].tobytes(), f"{what}: tick {t}"
        assert eng.get_state().tobytes() == st_end.tobytes(), what

    rpcs = Buf(S * max(N - 1, 1) * 56 * T, on_gpu)
    for kc in (kinds, None):                                           # class-dispatch kernel, kind-generic kernel
        eng.set_state(0, st0)
        dec = Buf(T * tb, on_gpu)
        eng.run_ticks_device(msgs.ptr, S, T, dec.ptr, rpcs.ptr, tick_counts=counts, kind_counts=kc)
        eng.synchronize()
        compare(dec, f"rgb_run_ticks_device (kind counts: {kc is not None})")
    eng.set_state(0, st0)                                              # one train launch over all ticks
    buckets = np.stack([np.bincount(train_bucket(m["kind"], m["flags"], m["server"], N),
                                    minlength=engine_mod.TRAIN_BUCKETS) for m in ticks]).astype(np.uint32)
    plan = eng.train_plan(buckets)
    stamps, dec = Buf(T * S, on_gpu), Buf(T * tb, on_gpu)
    eng.train_stamp_device(msgs.ptr, stamps.ptr, S, counts)
    eng.train_run_device(plan, 0, T, msgs.ptr, stamps.ptr, S, dec.ptr, rpcs.ptr, rpc_ring=T)
    eng.synchronize()
    flags, _ = eng.train_status()
    assert flags == 0
    compare(dec, "train launch")
    plan.close()


@pytest.mark.parametrize("G,N,T,seed", [(64, 3, 6, 71), (48, 5, 6, 72), (32, 8, 5, 73)])
def test_every_path_gives_the_same_answer_on_the_emulated_engine(emulated_engine, oracle_lib, G, N, T, seed):
    check_every_path(emulated_engine, oracle_lib, G, N, T, seed, False)


@pytest.mark.gpu
@pytest.mark.parametrize("G,N,T,seed", [(4096, 5, 8, 81), (2048, 3, 8, 82), (1024, 7, 6, 83)])
def test_every_path_gives_the_same_answer_on_the_gpu(oracle_lib, G, N, T, seed):
    from ra_amd import engine
    check_every_path(engine, oracle_lib, G, N, T, seed, True)
