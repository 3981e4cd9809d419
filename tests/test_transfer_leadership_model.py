"""A Python restatement of handle_leader({transfer_leadership, Target}, _) (src/ra_server.erl:996-1035), the other
roles' catch-all reply (:1186-1188, 1276-1278, 1655-1657) and the await condition transfer_leadership_condition/2
(:2235-2245) inside handle_await_condition/2 (:1916-1959), fuzzed on random states against the engine.

Where the reference re-processes the message in another role ({next_event, Msg}), the engine's one decision is
checked as two steps: the modelled role change, then the unchanged checker on the intermediate follower state (as
tests/test_election_model.py does).  request_vote_rpc, pre_vote_rpc, election_timeout and the ra_log events, which
the reference serves before any predicate (:1918-1931, 1946-1949), are compared with the checker twice: on the same
server awaiting COND_MISSING instead (the clauses do not look at the condition), and on the server as it is."""
import numpy as np
import pytest

from ra_amd import abi
import fuzz
from test_election_model import random_msg


def ra_log_next_index(row):                                           # src/ra_log.erl:1166-1174
    if int(row["first_index"]) <= int(row["last_index"]):
        return int(row["last_index"]) + 1
    if int(row["snapshot_index"]) != abi.UNDEF_INT:
        return int(row["snapshot_index"]) + 1
    return 0


def leader_transfer(row, target):
    """:996-1035 in the reference's clause order -> the reply code."""
    if target == int(row["self"]):
        return abi.CALL_ALREADY_LEADER                               # :996-1000
    if target >= abi.MAX_MEMBERS or not (int(row["present_mask"]) >> target) & 1:
        return abi.CALL_UNKNOWN_MEMBER                               # :1001-1007 (not is_map_key)
    if not (int(row["voter_mask"]) >> target) & 1:
        return abi.CALL_NON_VOTER                                    # :1012-1016
    if int(row["next_index"][target]) != ra_log_next_index(row):
        return abi.CALL_NOT_UP_TO_DATE                               # :1030-1033
    return abi.CALL_OK                                               # :1019-1029


def make_log_empty(st, s):
    """Neither a range nor a snapshot: ra_log:next_index/1 = 0 (src/ra_log.erl:1173-1174)."""
    st["first_index"][s], st["last_index"][s], st["last_term"][s] = 1, 0, 0
    st["n_runs"][s] = 0
    st["run_start"][s], st["run_term"][s] = 0, 0
    st["snapshot_index"][s] = st["snapshot_term"][s] = abi.UNDEF
    st["last_written_index"][s], st["last_written_term"][s] = 0, 0
    st["pending_first"][s] = 1
    st["commit_index"][s] = st["last_applied"][s] = 0


def random_transfer_states(rng, G, n, empty_logs=True):
    """fuzz.random_states (snapshots, empty ranges) with level peers and, for the call, some logs with neither."""
    st = fuzz.random_states(rng, G, n, max_runs=6)
    for s in range(len(st)):
        if empty_logs and rng.random() < 0.06:
            make_log_empty(st, s)
        for j in range(n):                                            # level peers: next_index = ra_log:next_index/1
            if rng.random() < 0.4:
                st["next_index"][s, j] = ra_log_next_index(st[s])
    return st


def check_leader_clause(eng, oracle_lib, n, seed):
    """Kind 16 to servers in every role: the leader's clauses, the unsupported_call reply, the drop of await_condition
    and the wal_down leader that can write again (back to leader, the call re-processed)."""
    rng = np.random.default_rng(seed)
    G = 120
    st = random_transfer_states(rng, G, n)
    S = len(st)
    wal = rng.random(S) < 0.1
    st["role"][wal] = abi.ROLE_AWAIT_CONDITION
    st["cond_reason"][wal] = abi.COND_WAL_DOWN_LEADER
    empty_leaders = [g * n for g in range(3)] if n >= 2 else []      # level with member 1 at next_index 0
    for s in empty_leaders:
        make_log_empty(st, s)
        wal[s] = False
        st["role"][s], st["self"][s] = abi.ROLE_LEADER, 0
        st["present_mask"][s] = st["voter_mask"][s] = (1 << n) - 1
        st["next_index"][s, 1] = 0
    eng.set_state(0, st)
    before = eng.get_state()
    msgs = np.zeros(S, dtype=abi.MSG_DTYPE)
    msgs["server"] = np.arange(S)
    msgs["kind"] = abi.MSG_TRANSFER_LEADERSHIP
    for s in range(S):
        row = before[s]
        lvl = [j for j in range(n) if int(row["next_index"][j]) == ra_log_next_index(row)]
        msgs["from"][s] = int(rng.choice([int(row["self"]), abi.NONE, min(n, 7), 7] + lvl * 3 + list(range(n))))
        if wal[s] and rng.random() < 0.6:
            msgs["flags"][s] = abi.MF_CAN_WRITE
    msgs["from"][empty_leaders] = 1
    dec, rpcs = eng.step(msgs)
    after = eng.get_state()
    assert len(rpcs) == 0
    seen = np.zeros(8, dtype=np.int64)
    for s in range(S):
        row0, row1, d, m = before[s], after[s], dec[s], msgs[s]
        role0, target = int(row0["role"]), int(m["from"])
        tag = f"N={n} server {s} role {role0} reason {int(row0['cond_reason'])} target {target}"
        fl = int(d["flags"])
        reprocess = role0 == abi.ROLE_AWAIT_CONDITION and wal[s] and int(m["flags"]) & abi.MF_CAN_WRITE
        if role0 == abi.ROLE_LEADER or reprocess:
            code = leader_transfer(row0, target)
            want_role = abi.ROLE_AWAIT_CONDITION if code == abi.CALL_OK else abi.ROLE_LEADER
            want = abi.F_CALL_REPLY | (abi.F_ROLE_CHANGED if want_role != role0 or reprocess else 0)
            want |= abi.F_REPROCESSED if reprocess else 0
            assert fl == want, (tag, hex(fl), hex(want))
            assert int(d["reply_next_index"]) == code, (tag, int(d["reply_next_index"]), code)
            assert int(d["reply_to"]) == (target if code == abi.CALL_OK else abi.NONE), tag
            mid = row0.copy()
            mid["role"] = want_role
            mid["cond_reason"] = abi.COND_TRANSFER_LEADERSHIP if code == abi.CALL_OK else abi.COND_NONE
            assert row1.tobytes() == mid.tobytes(), tag
            seen[code] += 1
        elif role0 == abi.ROLE_AWAIT_CONDITION:                       # the predicate is false: dropped (:1950-1959)
            assert fl == 0 and int(d["reply_to"]) == abi.NONE, (tag, hex(fl))
            assert row1.tobytes() == row0.tobytes(), tag
            seen[6] += 1
        else:                                                         # {error, {unsupported_call, Msg}}
            assert fl == abi.F_CALL_REPLY and int(d["reply_next_index"]) == abi.CALL_UNSUPPORTED, (tag, hex(fl))
            assert int(d["reply_to"]) == abi.NONE and row1.tobytes() == row0.tobytes(), tag
            seen[abi.CALL_UNSUPPORTED] += 1
        assert (int(d["reply_term"]), int(d["reply_last_index"]), int(d["reply_last_term"])) == (0, 0, 0), tag
        assert (int(d["commit_index"]), int(d["last_applied"])) == (int(row1["commit_index"]), int(row1["last_applied"]))
        assert int(d["role"]) == int(row1["role"]) and int(d["kind"]) == abi.MSG_TRANSFER_LEADERSHIP, tag
    if n == 1:                                                        # no other member: only self and strangers
        assert np.all(seen[[abi.CALL_ALREADY_LEADER, abi.CALL_UNKNOWN_MEMBER, abi.CALL_UNSUPPORTED, 6]] > 0), seen
        return
    assert np.all(seen[:7] > 0), seen
    # a level peer of an EMPTY log (no range, no snapshot: next_index 0) is up to date
    assert all(int(dec["reply_next_index"][s]) == abi.CALL_OK for s in empty_leaders)


COND_KINDS = [abi.MSG_AER, abi.MSG_AER, abi.MSG_AER, abi.MSG_HEARTBEAT_RPC, abi.MSG_REQUEST_VOTE, abi.MSG_PRE_VOTE_RPC,
              abi.MSG_ELECTION_TIMEOUT, abi.MSG_AWAIT_TIMEOUT, abi.MSG_VOTE_RESULT, abi.MSG_AER_REPLY,
              abi.MSG_PRE_VOTE_RESULT, abi.MSG_HEARTBEAT_REPLY, abi.MSG_WRITTEN, abi.MSG_SNAPSHOT_WRITTEN,
              abi.MSG_APPEND, abi.MSG_PIPELINE_RPCS, abi.MSG_CONSISTENT_QUERY, abi.MSG_TRANSFER_LEADERSHIP]
SERVED_FIRST = (abi.MSG_PRE_VOTE_RPC, abi.MSG_ELECTION_TIMEOUT, abi.MSG_WRITTEN, abi.MSG_SNAPSHOT_WRITTEN)


def one_group(states, sv, n, row):
    base = (sv // n) * n
    grp = states[base:base + n].copy()
    grp[sv - base] = row
    return grp, sv - base


def check_condition(eng, oracle_lib, n, seed):
    rng = np.random.default_rng(seed)
    G = 150
    st = random_transfer_states(rng, G, n, empty_logs=False)
    S = len(st)
    st["role"] = abi.ROLE_AWAIT_CONDITION
    st["cond_reason"] = abi.COND_TRANSFER_LEADERSHIP
    eng.set_state(0, st)
    before = eng.get_state()
    msgs = []
    for sv in range(S):
        row = before[sv]
        m = random_msg(rng, sv, row, n, COND_KINDS)
        k = int(m["kind"][0])
        if k == abi.MSG_AER and rng.random() < 0.5:
            m["term"] = int(row["current_term"]) + 1                  # the predicate's case, half of the time
        elif k == abi.MSG_WRITTEN:
            li = int(row["last_index"])
            m["a"], m["b"] = min(int(row["pending_first"]), li), li
            m["term"] = int(row["last_term"])
        elif k == abi.MSG_SNAPSHOT_WRITTEN:
            m["a"], m["b"] = int(row["last_applied"]), fuzz._term_at(row, int(row["last_applied"])) or 0
        elif k in (abi.MSG_TRANSFER_LEADERSHIP, abi.MSG_APPEND, abi.MSG_PIPELINE_RPCS, abi.MSG_CONSISTENT_QUERY,
                   abi.MSG_AWAIT_TIMEOUT):
            m["term"] = 0
        msgs.append(m[0])
    msgs = np.array(msgs, dtype=abi.MSG_DTYPE)
    dec, rpcs = eng.step(msgs)
    after = eng.get_state()
    seen = {"released": 0, "dropped": 0, "timeout": 0, "vote": 0, "served_first": 0}
    for m, d in zip(msgs, dec):
        sv = int(m["server"])
        row0, row1 = before[sv], after[sv]
        k, fl = int(m["kind"]), int(d["flags"])
        tag = f"N={n} server {sv} msg {m}"
        released = k == abi.MSG_AER and int(m["term"]) > int(row0["current_term"])       # :2235-2238
        if k == abi.MSG_REQUEST_VOTE or released:
            # :1918-1919 / :1950-1955: follower (no top-level transition_to), then the message again
            mid = row0.copy()
            mid["role"], mid["cond_reason"] = abi.ROLE_FOLLOWER, abi.COND_NONE
            mid["status_mask"], mid["backoff_mask"] = 0xFF, 0                # become(follower, ..) :2182-2192
            grp, i = one_group(before, sv, n, mid)
            two = oracle_lib.Oracle(1, n)
            two.set_state(0, grp)
            m2 = m.copy(); m2["server"] = i
            d2, _ = two.step(np.array([m2], dtype=abi.MSG_DTYPE))
            got = two.get_state()[i]
            two.close()
            if fl & abi.F_INVARIANT:
                assert int(d2["flags"][0]) & abi.F_INVARIANT and int(d2["invariant"][0]) == int(d["invariant"]), tag
                assert row1.tobytes() == row0.tobytes(), tag
                continue
            assert got.tobytes() == row1.tobytes(), (tag, [f for f in abi.SERVER_STATE_DTYPE.names
                                                           if got[f].tobytes() != row1[f].tobytes()])
            same = ~(abi.F_REPROCESSED | abi.F_ROLE_CHANGED | abi.F_LEADER_CHANGED)
            assert fl & abi.F_REPROCESSED and (fl & same) == (int(d2["flags"][0]) & same), (tag, hex(fl))
            for f in ("reply_to", "reply_term", "reply_next_index", "reply_last_index", "reply_last_term",
                      "commit_index", "last_applied", "heartbeat_to"):
                assert int(d[f]) == int(d2[f][0]), (tag, f)
            seen["vote" if k == abi.MSG_REQUEST_VOTE else "released"] += 1
        elif k in SERVED_FIRST:
            # served before the predicate: the checker on the same server awaiting another condition
            alt = row0.copy()
            alt["cond_reason"] = abi.COND_MISSING
            grp, i = one_group(before, sv, n, alt)
            two = oracle_lib.Oracle(1, n)
            two.set_state(0, grp)
            m2 = m.copy(); m2["server"] = i
            d2, _ = two.step(np.array([m2], dtype=abi.MSG_DTYPE))
            got = two.get_state()[i].copy()
            two.close()
            if int(got["role"]) == abi.ROLE_AWAIT_CONDITION:
                got["cond_reason"] = abi.COND_TRANSFER_LEADERSHIP
            d2 = d2.copy(); d2["server"] = sv
            assert got.tobytes() == row1.tobytes(), tag
            assert d2[0].tobytes() == d.tobytes(), (tag, d2[0], d)
            # and the checker holding the server as it is, in the transfer condition
            grp, i = one_group(before, sv, n, row0)
            two = oracle_lib.Oracle(1, n)
            two.set_state(0, grp)
            d3, _ = two.step(np.array([m2], dtype=abi.MSG_DTYPE))
            got = two.get_state()[i]
            two.close()
            d3 = d3.copy(); d3["server"] = sv
            assert got.tobytes() == row1.tobytes(), tag
            assert d3[0].tobytes() == d.tobytes(), (tag, d3[0], d)
            seen["served_first"] += 1
        elif k == abi.MSG_AWAIT_TIMEOUT:                              # :1932-1945 with the timeout map of :1027-1028
            want = row0.copy()
            want["role"], want["cond_reason"] = abi.ROLE_LEADER, abi.COND_NONE
            assert row1.tobytes() == want.tobytes(), tag
            assert fl == abi.F_ROLE_CHANGED and int(d["reply_to"]) == abi.NONE, (tag, hex(fl))
            seen["timeout"] += 1
        else:                                                         # the predicate is false: dropped (:1956-1959)
            assert row1.tobytes() == row0.tobytes(), tag
            assert fl == 0 and int(d["reply_to"]) == abi.NONE and int(d["n_rpcs"]) == 0, (tag, hex(fl))
            seen["dropped"] += 1
    assert all(v > 3 for v in seen.values()), seen


NS = [(1, 11), (2, 12), (3, 13), (5, 14), (7, 15), (8, 16)]


@pytest.mark.parametrize("n,seed", NS)
def test_transfer_call_matches_the_model_on_the_emulated_engine(emulated_engine, oracle_lib, n, seed):
    with emulated_engine.RaGpuBatch(120, n, ring_capacity=120 * n, ring_slots=2, max_runs=16) as eng:
        check_leader_clause(eng, oracle_lib, n, 9100 + seed)


@pytest.mark.parametrize("n,seed", NS)
def test_transfer_condition_matches_the_model_on_the_emulated_engine(emulated_engine, oracle_lib, n, seed):
    with emulated_engine.RaGpuBatch(150, n, ring_capacity=150 * n, ring_slots=2, max_runs=16) as eng:
        check_condition(eng, oracle_lib, n, 9200 + seed)


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed", NS)
def test_transfer_call_matches_the_model_on_the_gpu(oracle_lib, n, seed):
    from ra_amd import engine
    with engine.RaGpuBatch(120, n, ring_capacity=120 * n, ring_slots=2, max_runs=16) as eng:
        check_leader_clause(eng, oracle_lib, n, 9300 + seed)


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed", NS)
def test_transfer_condition_matches_the_model_on_the_gpu(oracle_lib, n, seed):
    from ra_amd import engine
    with engine.RaGpuBatch(150, n, ring_capacity=150 * n, ring_slots=2, max_runs=16) as eng:
        check_condition(eng, oracle_lib, n, 9400 + seed)
