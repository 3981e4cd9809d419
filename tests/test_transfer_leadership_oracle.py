"""{transfer_leadership, Target} and its await condition refereed by the sequential CPU checker (oracle/ra_oracle.c) in
every fuzz path: the checker restates handle_leader/2's clause (src/ra_server.erl:996-1035), the other roles' catch-all
reply (:1186-1188, 1276-1278, 1655-1657) and transfer_leadership_condition/2 inside handle_await_condition/2
(:1916-1959, 2235-2245) from the reference source, independently of the kernels.

a. the referees agree: the checker passes the transcribed vectors and the Python model of
   test_transfer_leadership_model.py, before either judges the device;
b. random ticks, one message per server, transfers mixed in (fuzz.random_states / random_msgs with transfers=);
c. several messages per server in one rgb_submit -- sub-tick rounds, one fused train, RGB_CFG_ROUNDS_PER_LAUNCH -- and
   hand-built batches for what follows an accepted transfer inside one batch;
d. the device-resident paths (rgb_run_ticks_device with and without kind counts, one train launch) with the checker's
   decisions as the expected values.

Decisions (those that carry RGB_F_INVARIANT like the rest), sorted rpc records and the full state must be byte-identical
to the checker's.  A test that never reaches a clause proves nothing: Coverage counts, from the checker's decisions
alone, every reply code of the call and every way a server leaves or stays in the transfer condition, and each test
asserts what it saw.  Each test runs on the CPU emulation of the HIP sources and, under -m gpu, on the MI355X."""
import numpy as np
import pytest

from ra_amd import abi
from ra_amd import effects as fx
import fuzz
import test_transfer_leadership as TL
import test_transfer_leadership_model as TM
from test_gpu_parity import assert_same

LOG_EVENTS = (abi.MSG_WRITTEN, abi.MSG_SNAPSHOT_WRITTEN)


class Coverage:
    """What the checker's decisions say was reached.  A server awaits the transfer condition if it was uploaded so or
    accepted a call (RGB_CALL_OK), until a decision shows another role or a re-processed message."""
    KEYS = ("released", "timed_out", "dropped", "vote_reprocessed", "log_event", "pre_vote_rpc", "election_timeout")

    def __init__(self):
        self.codes = set()
        self.n = dict.fromkeys(self.KEYS + ("accepted_then_more",), 0)

    def batch(self, st_before, msgs, dec):
        """st_before: the states the batch was applied to; msgs / dec in submission order (any number per server)."""
        waits = ((st_before["role"] == abi.ROLE_AWAIT_CONDITION) &
                 (st_before["cond_reason"] == abi.COND_TRANSFER_LEADERSHIP)).tolist()
        fresh = set()                                                 # accepted a call in THIS batch
        rows = zip(msgs["server"].tolist(), msgs["kind"].tolist(), dec["flags"].tolist(), dec["role"].tolist(),
                   dec["reply_next_index"].tolist())
        for s, kind, fl, role, code in rows:
            if kind == abi.MSG_NOP or fl & abi.F_INVARIANT:
                continue
            if waits[s]:
                if s in fresh:
                    self.n["accepted_then_more"] += 1
                    fresh.discard(s)
                if kind == abi.MSG_AER and fl & abi.F_REPROCESSED:
                    self.n["released"] += 1
                elif kind == abi.MSG_AWAIT_TIMEOUT:
                    assert role == abi.ROLE_LEADER and fl == abi.F_ROLE_CHANGED, (s, role, hex(fl))
                    self.n["timed_out"] += 1
                elif kind == abi.MSG_REQUEST_VOTE:
                    assert fl & abi.F_REPROCESSED, (s, hex(fl))
                    self.n["vote_reprocessed"] += 1
                elif kind in LOG_EVENTS:
                    self.n["log_event"] += 1
                elif kind == abi.MSG_PRE_VOTE_RPC:
                    self.n["pre_vote_rpc"] += 1
                elif kind == abi.MSG_ELECTION_TIMEOUT:
                    self.n["election_timeout"] += 1
                else:
                    assert fl == 0 and role == abi.ROLE_AWAIT_CONDITION, (s, kind, hex(fl))
                    self.n["dropped"] += 1
                waits[s] = role == abi.ROLE_AWAIT_CONDITION and not fl & abi.F_REPROCESSED
            elif kind == abi.MSG_TRANSFER_LEADERSHIP and fl & abi.F_CALL_REPLY:
                self.codes.add(code)
                if code == abi.CALL_OK:
                    assert role == abi.ROLE_AWAIT_CONDITION, (s, role)
                    waits[s] = True
                    fresh.add(s)

    def check(self, n_members, same_batch=False):
        if n_members == 1:            # no other member: only already_leader / unknown_member, nobody ever waits
            assert self.codes == {abi.CALL_ALREADY_LEADER, abi.CALL_UNKNOWN_MEMBER, abi.CALL_UNSUPPORTED}, self.codes
        else:
            assert self.codes == set(range(6)), self.codes
        for k in self.KEYS:
            assert self.n[k] > 0, (k, self.n)
        if same_batch:
            assert self.n["accepted_then_more"] > 0, self.n


# ------------------------------------------------------------------------------------------ a. the referees agree
def test_the_checker_passes_the_transcribed_vectors(oracle_lib):
    cpu = oracle_lib.Oracle(1, 3)
    TL.run_vectors(cpu)
    cpu.close()


@pytest.mark.parametrize("n,seed", TM.NS)
def test_the_checker_agrees_with_the_model_of_the_call(oracle_lib, n, seed):
    cpu = oracle_lib.Oracle(120, n)
    TM.check_leader_clause(cpu, oracle_lib, n, 9500 + seed)
    cpu.close()


@pytest.mark.parametrize("n,seed", TM.NS)
def test_the_checker_agrees_with_the_model_of_the_condition(oracle_lib, n, seed):
    cpu = oracle_lib.Oracle(150, n)
    TM.check_condition(cpu, oracle_lib, n, 9620 + seed)
    cpu.close()


def test_the_checker_refuses_an_unknown_condition(oracle_lib):
    """ora_set_state refuses cond_reason > RGB_COND_TRANSFER_LEADERSHIP as rgb_upload_state does, as a whole."""
    cpu = oracle_lib.Oracle(2, 3)
    st = abi.empty_server_states(2, 3)
    st["role"][1] = abi.ROLE_AWAIT_CONDITION
    st["cond_reason"][1] = abi.COND_TRANSFER_LEADERSHIP
    cpu.set_state(0, st)
    assert cpu.get_state().tobytes() == st.tobytes()
    bad = st.copy()
    bad["current_term"][0] = 9
    bad["cond_reason"][4] = abi.COND_TRANSFER_LEADERSHIP + 1
    with pytest.raises(ValueError):
        cpu.set_state(0, bad)
    assert cpu.get_state().tobytes() == st.tobytes()
    cpu.close()


def test_the_default_random_stream_has_not_moved():
    """transfers= is opt-in: with the defaults the generators draw exactly what they drew before (smoke() and every
    recorded seed depend on it).  The hash was taken on the commit before the argument existed."""
    import hashlib
    rng = np.random.default_rng(7)
    s = fuzz.random_states(rng, 50, 5)
    m = fuzz.random_msgs(rng, s, 5)
    assert hashlib.sha256(s.tobytes() + m.tobytes()).hexdigest() == \
        "2c0a3f4b20267a074f768d75381fb44a2997eb649ec09e93b7d2d83281c4f127"
    assert not np.any(m["kind"] == abi.MSG_TRANSFER_LEADERSHIP)
    assert not np.any(s["cond_reason"] == abi.COND_TRANSFER_LEADERSHIP)


# ------------------------------------------------------------------------------------------------- b. random ticks
def transfer_states(rng, G, N, deep, wal_down):
    st = fuzz.random_states(rng, G, N, max_runs=16 if deep else 6, backlog=60 if deep else 24, transfers=0.6)
    if wal_down:
        # a tenth of the servers waits in one of the two wal_down conditions: a call that reaches one is dropped, or --
        # with RGB_MF_CAN_WRITE -- re-processed by the leader / the follower the condition returns to
        pick = rng.random(G * N) < 0.1
        st["role"][pick] = abi.ROLE_AWAIT_CONDITION
        st["cond_reason"][pick] = rng.choice([abi.COND_WAL_DOWN, abi.COND_WAL_DOWN_LEADER], size=int(pick.sum()))
    return st


def transfer_tick(rng, cur, N, wal_down, frac=0.9):
    m = fuzz.random_msgs(rng, cur, N, frac=frac, transfers=0.2)
    if wal_down:
        m["flags"] |= np.where(rng.random(len(m)) < 0.5, abi.MF_CAN_WRITE, 0).astype(m["flags"].dtype)
    return m


def check_random_ticks(engine, oracle_lib, N, G, seed, deep, wal_down, ticks=5):
    rng = np.random.default_rng(seed)
    st = transfer_states(rng, G, N, deep, wal_down)
    cpu = oracle_lib.Oracle(G, N, max_runs=16)                        # bounded like the device
    cpu.set_state(0, st)
    cov = Coverage()
    with engine.RaGpuBatch(G, N, ring_capacity=max(4096, G * N), ring_slots=2, max_runs=16) as gpu:
        gpu.set_state(0, st)
        for t in range(ticks):
            cur = cpu.get_state()
            msgs = transfer_tick(rng, cur, N, wal_down)
            do, ro = cpu.step(msgs)
            dg, rg = gpu.step(msgs)
            assert_same(f"N={N} seed {seed} tick {t}", dg, rg, gpu.get_state(), do, ro, cpu.get_state())
            cov.batch(cur, msgs, do)
    cpu.close()
    cov.check(N)


# (N, servers' groups, seed): shallow / deep run tables and with / without wal_down servers alternate over the cases of
# one group size, so that all four combinations run for every N
TICK_CASES = [(N, G, 7000 + 10 * N + k, bool(k & 1), bool(k & 2))
              for N, G in ((1, 1500), (2, 750), (3, 500), (5, 300), (7, 220), (8, 190)) for k in range(4)]


@pytest.mark.parametrize("N,G,seed,deep,wal_down", TICK_CASES)
def test_random_ticks_with_transfers_on_the_emulated_engine(emulated_engine, oracle_lib, N, G, seed, deep, wal_down):
    check_random_ticks(emulated_engine, oracle_lib, N, G, seed, deep, wal_down)


@pytest.mark.gpu
@pytest.mark.parametrize("N,G,seed,deep,wal_down", [(N, 3 * G, seed + 500, deep, wal) for N, G, seed, deep, wal in TICK_CASES])
def test_random_ticks_with_transfers_on_the_gpu(oracle_lib, N, G, seed, deep, wal_down):
    from ra_amd import engine
    check_random_ticks(engine, oracle_lib, N, G, seed, deep, wal_down)


# ------------------------------------------------------------------------- c. several messages per server in one submit
def check_rounds(engine, oracle_lib, N, G, seed, cfg_flags, want_trains, batches=2):
    rng = np.random.default_rng(seed)
    deep = seed % 2 == 1
    st = transfer_states(rng, G, N, deep, wal_down=True)
    cpu = oracle_lib.Oracle(G, N, max_runs=16)
    cpu.set_state(0, st)
    cov = Coverage()
    with engine.RaGpuBatch(G, N, ring_capacity=65536, ring_slots=2, max_runs=16, flags=cfg_flags) as gpu:
        gpu.set_state(0, st)
        for b in range(batches):
            cur = cpu.get_state()
            msgs = np.concatenate([transfer_tick(rng, cur, N, True) for _ in range(4)])
            msgs = msgs[msgs["kind"] != abi.MSG_NOP]
            rng.shuffle(msgs)
            assert len(msgs) >= 4096
            do, ro = cpu.step(msgs)
            dg, rg = gpu.step(msgs)
            assert_same(f"N={N} seed {seed} flags {cfg_flags} batch {b}", dg, rg, gpu.get_state(), do, ro, cpu.get_state())
            cov.batch(cur, msgs, do)
        if want_trains:
            assert gpu.submit_trains() >= 1
        else:
            assert gpu.submit_trains() == 0
    cpu.close()
    cov.check(N, same_batch=True)


ROUND_CFGS = [(0, False), (abi.CFG_SUBMIT_TRAINS, True), (abi.CFG_SUBMIT_TRAINS | abi.CFG_ROUNDS_PER_LAUNCH, False)]
ROUND_CASES = [(N, G, 7300 + 10 * N + k, fl, tr) for N, G in ((3, 1800), (5, 1100), (7, 800))
               for k, (fl, tr) in enumerate(ROUND_CFGS)]


@pytest.mark.parametrize("N,G,seed,cfg_flags,want_trains", ROUND_CASES)
def test_rounds_of_one_submit_with_transfers_on_the_emulated_engine(emulated_engine, oracle_lib, N, G, seed, cfg_flags,
                                                                    want_trains):
    check_rounds(emulated_engine, oracle_lib, N, G, seed, cfg_flags, want_trains)


@pytest.mark.gpu
@pytest.mark.parametrize("N,G,seed,cfg_flags,want_trains", [(N, G, seed + 500, fl, tr) for N, G, seed, fl, tr in ROUND_CASES])
def test_rounds_of_one_submit_with_transfers_on_the_gpu(oracle_lib, N, G, seed, cfg_flags, want_trains):
    from ra_amd import engine
    check_rounds(engine, oracle_lib, N, G, seed, cfg_flags, want_trains, batches=3)


def level_leader(G, N):
    """Every group: member 0 leads term 5 over the log of base_state/2 (test/ra_server_SUITE.erl:4151-4192), every peer
    level with it (next_index 4 = ra_log:next_index/1, match_index 3), members 1.. are its followers."""
    st = abi.empty_server_states(G, N)
    for s in range(G * N):
        abi.set_log(st, s, [(0, 0), (1, 1), (2, 3), (3, 5)], last_written=(3, 5))
        st["current_term"][s] = 5
        st["commit_index"][s] = st["last_applied"][s] = 3
        st["leader_id"][s] = 0
        st["next_index"][s, :N] = 4
        st["match_index"][s, :N] = 3
        st["commit_index_sent"][s, :N] = 3
        if s % N == 0:
            st["role"][s] = abi.ROLE_LEADER
    return st


def hand_built_batch(G, N):
    """Four scenarios for the leader of a group, one per group in turn, all inside ONE batch (the groups' messages
    interleaved, each leader's in order):
      0  call accepted, then append_entries_reply + command + pipeline_rpcs: all dropped, nothing committed, no rpcs
      1  call accepted, then an append_entries_rpc of term 6: released to follower, re-processed, the reply sent
      2  call accepted, then await_condition_timeout, then a command: leader again, the command appended
      3  two calls: the second is dropped unanswered"""
    per_group = []
    for g in range(G):
        s = g * N
        call = fx.encode(s, fx.TransferLeadership(1))
        k = g % 4
        if k == 0:
            seq = [call,
                   fx.encode(s, fx.AppendEntriesReply(5, True, 4, 3, 5), from_slot=1),
                   fx.encode(s, fx.Commands(2)),
                   fx.encode(s, fx.PIPELINE_RPCS)]
        elif k == 1:
            seq = [call, fx.encode(s, fx.AppendEntriesRpc(6, 1, 3, 3, 5))]
        elif k == 2:
            seq = [call, fx.encode(s, fx.AWAIT_CONDITION_TIMEOUT), fx.encode(s, fx.Commands(2))]
        else:
            seq = [call, fx.encode(s, fx.TransferLeadership(2))]
        per_group.append(seq)
    out = []
    for r in range(4):                                                # round r: every leader's r-th message
        out += [seq[r] for seq in per_group if r < len(seq)]
    return np.array(out, dtype=abi.MSG_DTYPE)


def check_hand_built(engine, oracle_lib, cfg_flags, G, N=3):
    st = level_leader(G, N)
    msgs = hand_built_batch(G, N)
    cpu = oracle_lib.Oracle(G, N, max_runs=16)
    cpu.set_state(0, st)
    do, ro = cpu.step(msgs)
    so = cpu.get_state()
    cpu.close()
    # what the reference does, stated on the checker's answer; the device must then equal it byte for byte
    by_server = {}
    for m, d in zip(msgs, do):
        by_server.setdefault(int(m["server"]), []).append(d)
    rpcs_of = set(int(r["server"]) for r in ro)
    for g in range(G):
        s, k = g * N, g % 4
        ds, row = by_server[s], so[s]
        first = ds[0]
        assert int(first["flags"]) == abi.F_CALL_REPLY | abi.F_ROLE_CHANGED and int(first["reply_next_index"]) == abi.CALL_OK
        assert int(first["reply_to"]) == 1 and int(first["role"]) == abi.ROLE_AWAIT_CONDITION
        if k == 0:
            assert all(int(d["flags"]) == 0 and int(d["n_rpcs"]) == 0 for d in ds[1:]), ds
            assert int(row["role"]) == abi.ROLE_AWAIT_CONDITION and int(row["cond_reason"]) == abi.COND_TRANSFER_LEADERSHIP
            assert (int(row["last_index"]), int(row["commit_index"]), int(row["match_index"][1])) == (3, 3, 3)
            assert s not in rpcs_of
        elif k == 1:
            fl = int(ds[1]["flags"])
            assert fl & abi.F_REPROCESSED and fl & abi.F_REPLY and fl & abi.F_REPLY_SUCCESS, hex(fl)
            assert int(ds[1]["reply_to"]) == 1 and int(ds[1]["reply_term"]) == 6
            assert (int(row["role"]), int(row["current_term"]), int(row["leader_id"])) == (abi.ROLE_FOLLOWER, 6, 1)
        elif k == 2:
            assert int(ds[1]["flags"]) == abi.F_ROLE_CHANGED and int(ds[1]["role"]) == abi.ROLE_LEADER
            assert not int(ds[2]["flags"]) & (abi.F_UNHANDLED | abi.F_INVARIANT)
            assert (int(row["role"]), int(row["cond_reason"]), int(row["last_index"])) == (abi.ROLE_LEADER, abi.COND_NONE, 5)
        else:
            assert int(ds[1]["flags"]) == 0 and int(ds[1]["reply_to"]) == abi.NONE     # dropped: no {reply, _}
            assert int(row["role"]) == abi.ROLE_AWAIT_CONDITION
    with engine.RaGpuBatch(G, N, ring_capacity=65536, ring_slots=2, max_runs=16, flags=cfg_flags) as gpu:
        gpu.set_state(0, st)
        dg, rg = gpu.step(msgs)
        assert_same(f"hand-built batch, flags {cfg_flags}", dg, rg, gpu.get_state(), do, ro, so)
        if cfg_flags == abi.CFG_SUBMIT_TRAINS and len(msgs) >= 4096:
            assert gpu.submit_trains() == 1


# 1600 groups: 4400 messages in four rounds, enough for RGB_CFG_SUBMIT_TRAINS to fuse them; 8 groups: the small-batch form
@pytest.mark.parametrize("cfg_flags,G", [(0, 8), (0, 1600), (abi.CFG_SUBMIT_TRAINS, 1600)])
def test_what_follows_an_accepted_transfer_in_one_batch_on_the_emulated_engine(emulated_engine, oracle_lib, cfg_flags, G):
    check_hand_built(emulated_engine, oracle_lib, cfg_flags, G)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_flags,G", [(0, 8), (0, 1600), (abi.CFG_SUBMIT_TRAINS, 1600)])
def test_what_follows_an_accepted_transfer_in_one_batch_on_the_gpu(oracle_lib, cfg_flags, G):
    from ra_amd import engine
    check_hand_built(engine, oracle_lib, cfg_flags, G)


# ------------------------------------------------------------------------------------- d. the device-resident paths
def check_device_paths(engine, oracle_lib, G, N, T, seed, on_gpu):
    from ra_amd import engine as engine_mod
    rng = np.random.default_rng(seed)
    S = G * N
    st0 = transfer_states(rng, G, N, deep=False, wal_down=True)
    cpu = oracle_lib.Oracle(G, N, max_runs=16)
    cpu.set_state(0, st0)
    cov = Coverage()
    ticks, want_dec = [], []
    for t in range(T):                                                # the checker alone makes the expected values
        cur = cpu.get_state()
        m = transfer_tick(rng, cur, N, True)
        m = m[m["kind"] != abi.MSG_NOP]
        m = m[np.argsort(engine_mod.train_bucket(m["kind"], m["flags"], m["server"], N), kind="stable")]
        do, _ = cpu.step(m)
        cov.batch(cur, m, do)
        ticks.append(m)
        want_dec.append(do)
    st_end = cpu.get_state()
    cpu.close()
    cov.check(N)
    eng = engine.RaGpuBatch(G, N, max_runs=16, ring_slots=2, ring_capacity=S)
    TL.replay_on_the_device_paths(eng, S, N, st0, ticks, want_dec, st_end, on_gpu)
    eng.close()


@pytest.mark.parametrize("G,N,T,seed", [(600, 3, 5, 7601), (400, 5, 5, 7602), (280, 7, 5, 7603), (250, 8, 5, 7604),
                                        (1000, 2, 5, 7605), (2000, 1, 5, 7606)])
def test_device_resident_paths_against_the_checker_on_the_emulated_engine(emulated_engine, oracle_lib, G, N, T, seed):
    check_device_paths(emulated_engine, oracle_lib, G, N, T, seed, False)


@pytest.mark.gpu
@pytest.mark.parametrize("G,N,T,seed", [(4096, 5, 8, 7701), (2048, 3, 8, 7702), (1024, 7, 6, 7703), (1024, 8, 6, 7704),
                                        (2048, 2, 6, 7705), (4096, 1, 6, 7706)])
def test_device_resident_paths_against_the_checker_on_the_gpu(oracle_lib, G, N, T, seed):
    from ra_amd import engine
    check_device_paths(engine, oracle_lib, G, N, T, seed, True)
