"""The quorum term gate answered from the hot row (packed-word bit PK_CANON_SH, quorum_term_gate in rgb_kernels.hip).

A success reply at a leader and a leader's written event compute the agreed index p and ask whether its term is the
current term (Raft 5.4.2).  On a row whose run table is canonical -- run terms and starts strictly increasing, run 0
starting at or below first_index -- and whose last-run term is not above current_term, a p inside the range and below
the last run's start cannot pass the gate, and the kernels say so without the table; the success-reply rows of a train
launch do not even fetch the table's first line.  Everything else walks the table as before.

States are built by hand, one class per group (the letters are the issue's):
  (a) canonical table, 12 runs, p below the run before the last and inside the first eight runs;
  (b) the same with p behind the eighth run (a table of more than ten runs);
  (c) an OLD run carries current_term (terms not increasing: the bit must be clear) and p lands in it: commit moves;
  (d) canonical table whose last-run term is ABOVE current_term, p in an old run of the current term: commit moves;
  (e) snapshot_index == p and snapshot_term == current_term, p NOT answered by the table: commit moves through the
      snapshot clause.  The issue names "p inside the range but below the oldest run's start".  No such state can be
      built: rgb_upload_state and the oracle's set_state both refuse a range whose first run does not start at
      first_index (test_range_below_the_oldest_run_is_refused), and no message makes one (push_segment, compaction and
      overflow keep run 0 at or below first_index).  The case that exists is p = first_index - 1 = snapshot_index;
  (f) a follower is fed an append_entries_rpc whose entries LOWER the term (the push clears the bit), is elected by an
      election_timeout (sole voter: pre_vote, candidate and leader in one message), then receives a success reply whose
      p lies in the old run that carries the new current term: commit moves;
  (g) 264 groups x 5: shard 0 holds 33 leaders = one full 32-lane reply slice plus a one-lane tail, rows alternating
      (a) and (c).
Before any engine runs the test computes, from its own inputs, that every class holds a message whose p lies in the
region the class names.  Expected decisions, states and checksums come from the oracle alone.  Every stream runs
through the kind-generic per-tick kernel, the per-tick class kernel and a train launch in the default and in the
persistent form (on the block emulation, which has one XCC, both are the persistent kernel; on the device the default
is the dealt kernel)."""
import numpy as np
import pytest

from ra_amd import abi
from test_train import Buf

UNDEF = abi.UNDEF_INT


# ------------------------------------------------------------------------------------------------ state builders --
def _runs(n, length=3, first=1, terms=None):
    terms = list(range(1, n + 1)) if terms is None else list(terms)
    return [(first + length * k, terms[k]) for k in range(n)]


def _leader(st, s, N, runs, li, ct, x, ci=2, first=None, snapshot=None, lwi=None, reply_peer=True):
    """Server s (member 0 of its group) leads in term ct over the log `runs` .. li.  The members 1 .. quorum-1 match x
    (member 1 only once its reply has been counted when reply_peer), the leader has written up to lwi: with lwi >= x
    the agreed index is x."""
    r = st[s:s + 1]
    me = s % N
    r["first_index"] = runs[0][0] if first is None else first
    r["last_index"], r["last_term"] = li, runs[-1][1]
    r["n_runs"] = len(runs)
    for k, (a, t) in enumerate(runs):
        st["run_start"][s, k], st["run_term"][s, k] = a, t
    lwi = li if lwi is None else lwi
    r["last_written_index"] = lwi
    r["last_written_term"] = _term_at(runs, lwi)
    r["pending_first"] = lwi + 1
    if snapshot is not None:
        r["snapshot_index"], r["snapshot_term"] = snapshot
    r["current_term"] = ct
    r["commit_index"] = r["last_applied"] = ci
    r["role"], r["leader_id"], r["voted_for"] = abi.ROLE_LEADER, me, me
    q = N // 2 + 1
    for j in range(N):
        st["next_index"][s, j] = li + 1
        st["commit_index_sent"][s, j] = ci
        st["match_index"][s, j] = x if (j != me and j < q and not (reply_peer and j == 1)) else 0


def _term_at(runs, idx):
    t = None
    for a, tt in runs:
        if a <= idx:
            t = tt
    return t


def _reply(s, N, peer, term, match):
    m = np.zeros(1, dtype=abi.MSG_DTYPE)
    m["server"], m["kind"], m["from"], m["flags"], m["term"] = s, abi.MSG_AER_REPLY, peer, abi.MF_SUCCESS, term
    m["a"], m["b"] = match + 1, match
    return m


def _written(s, term, a, b):
    m = np.zeros(1, dtype=abi.MSG_DTYPE)
    m["server"], m["kind"], m["from"], m["term"], m["a"], m["b"] = s, abi.MSG_WRITTEN, abi.NONE, term, a, b
    return m


# ---------------------------------------------------------------------------- the model the coverage check uses --
def _agreed(st_row, N, lwi, counted=None):
    """agreed_commit over the voters' match indexes (the leader's own slot left out) and its last written index."""
    me = int(st_row["self"])
    v = [lwi]
    for j in range(N):
        if j == me or not (int(st_row["present_mask"]) >> j) & 1 or not (int(st_row["voter_mask"]) >> j) & 1:
            continue
        mi = int(st_row["match_index"][j])
        if counted is not None and counted[0] == j:
            mi = max(mi, counted[1])
        v.append(mi)
    return sorted(v, reverse=True)[len(v) // 2]


def _facts(runs, first, li, ct, p, si=UNDEF, stm=UNDEF):
    starts, terms = [a for a, _ in runs], [t for _, t in runs]
    inc = all(terms[k] < terms[k + 1] and starts[k] < starts[k + 1] for k in range(len(runs) - 1))
    idx = max([k for k, a in enumerate(starts) if a <= p], default=-1)
    return dict(canonical=inc and starts[0] <= first, increasing=inc, in_range=first <= p <= li, n=len(runs),
                below_prev=len(runs) >= 3 and p < starts[-2], run=idx, term=terms[idx] if idx >= 0 else None,
                lrt_le_ct=terms[-1] <= ct, snap=(si == p and stm == ct))


def _class_of(f, ct):
    """The issue's class of a message whose agreed index has the facts f (None: none of them)."""
    if not f["in_range"]:
        return "e" if (f["snap"] and f["run"] < 0) else None
    if f["run"] < 0:
        return None
    if not f["below_prev"]:
        return None
    if not f["lrt_le_ct"]:
        return "d"
    if not f["increasing"]:
        return "c" if f["term"] == ct else None
    if f["canonical"] and 3 <= f["n"] <= 16:
        return "b" if (f["run"] >= 8 and f["n"] > 10) else "a"
    return None


CASES = {  # class -> (runs, last index, current term, x, first_index, snapshot)
    "a": (_runs(12), 36, 12, 8, None, None),
    "b": (_runs(12), 36, 12, 26, None, None),
    "c": (_runs(6, terms=[1, 6, 2, 3, 4, 5]), 18, 6, 5, None, None),
    "d": (_runs(4, terms=[1, 3, 4, 9]), 12, 3, 5, None, None),
    "e": (_runs(3, first=10), 18, 3, 9, None, (9, 3)),
}


def _scenario(N):
    """8 groups x N, 3 ticks.  Returns (states, ticks, classes seen by the numpy model)."""
    G = 8
    st = abi.empty_server_states(G, N)
    seen = {}
    t0, t1, t2 = [], [], []
    layout = [("a", "reply"), ("b", "reply"), ("c", "reply"), ("d", "reply"), ("e", "reply"), ("a", "written"), ("c", "written")]
    for g, (cls, how) in enumerate(layout):
        runs, li, ct, x, first, snap = CASES[cls]
        s = g * N
        first_i = runs[0][0] if first is None else first
        if how == "reply":
            _leader(st, s, N, runs, li, ct, x, first=first, snapshot=snap)
            t0.append(_reply(s, N, 1, ct, x))
            p = _agreed(st[s], N, li, counted=(1, x))
        else:
            _leader(st, s, N, runs, li, ct, x, first=first, snapshot=snap, lwi=li - 1, reply_peer=False)
            t0.append(_written(s, runs[-1][1], li, li))
            p = _agreed(st[s], N, li)
        f = _facts(runs, first_i, li, ct, p, *(snap or (UNDEF, UNDEF)))
        got = _class_of(f, ct)
        assert got == cls, (cls, how, p, f)
        seen.setdefault(got, set()).add(how)
        # later ticks: the same question again from further members (the row has moved on: not part of the coverage claim)
        t1.append(_reply(s, N, 2, ct, x))
        t2.append(_reply(s, N, N - 1, ct, x + 1))
    # (f): member 1 of group 7, the group's only voter
    s = 7 * N + 1
    runs = [(1, 1), (4, 2), (7, 9)]
    r = st[s:s + 1]
    r["first_index"], r["last_index"], r["last_term"], r["n_runs"] = 1, 9, 9, 3
    for k, (a, t) in enumerate(runs):
        st["run_start"][s, k], st["run_term"][s, k] = a, t
    r["last_written_index"], r["last_written_term"], r["pending_first"] = 8, 9, 9
    r["current_term"], r["commit_index"], r["last_applied"] = 8, 2, 2
    r["leader_id"], r["voter_mask"] = 0, 1 << 1
    aer = np.zeros(1, dtype=abi.MSG_DTYPE)
    aer["server"], aer["kind"], aer["from"], aer["term"], aer["a"], aer["b"], aer["c"] = s, abi.MSG_AER, 0, 8, 9, 9, 2
    aer["n_entries"], aer["n_run0"], aer["run0_term"], aer["run1_term"] = 4, 2, 5, 6
    t0.append(aer)
    et = np.zeros(1, dtype=abi.MSG_DTYPE)
    et["server"], et["kind"], et["from"], et["c"] = s, abi.MSG_ELECTION_TIMEOUT, abi.NONE, 77
    t1.append(et)
    t2.append(_reply(s, N, 0, 9, 13))
    # the model: the rpc appends (10, 5) and (12, 6) behind the run of term 9, the election makes the term 9, the only
    # voter's written index (8) is the agreed index
    runs_f = runs + [(10, 5), (12, 6)]
    f = _facts(runs_f, 1, 13, 9, _agreed(st[s], N, 8))
    assert runs_f[-2][1] < runs[-1][1], "the rpc's entries lower the term"
    assert _class_of(f, 9) == "c" and not f["increasing"] and f["term"] == 9, f
    seen.setdefault("f", set()).add("reply")
    assert set(seen) == set("abcdef"), seen
    assert seen["a"] == {"reply", "written"} and seen["c"] == {"reply", "written"}
    return st, [np.concatenate(t) for t in (t0, t1, t2)], seen


def _scenario_slice():
    """264 groups x 5, 2 ticks: every leader gets a success reply; shard 0 (groups 0, 8, ..: 33 of them) is one full
    32-lane slice and a one-lane tail, rows alternating (a) and (c)."""
    G, N = 264, 5
    st = abi.empty_server_states(G, N)
    t0, t1, cls_of_group = [], [], []
    for g in range(G):
        cls = "a" if (g // 8) % 2 == 0 else "c"
        runs, li, ct, x, first, snap = CASES[cls]
        s = g * N
        _leader(st, s, N, runs, li, ct, x)
        t0.append(_reply(s, N, 1, ct, x))
        t1.append(_reply(s, N, 2, ct, x + 1))
        f = _facts(runs, runs[0][0], li, ct, _agreed(st[s], N, li, counted=(1, x)))
        assert _class_of(f, ct) == cls
        cls_of_group.append(cls)
    shard0 = [cls_of_group[g] for g in range(0, G, 8)]
    assert len(shard0) == 33 and set(shard0[:32]) == {"a", "c"}, "(g): one 32-lane slice mixes (a) and (c), plus a tail"
    return st, [np.concatenate(t0), np.concatenate(t1)]


def _scenario_overflow():
    """8 groups x 5, 2 ticks: a canonical leader row with a FULL table (16 runs) in a newer term appends (the 17th run:
    RGB_F_RUNS_OVERFLOW drops run 0 and moves first_index), then a success reply asks the gate."""
    G, N = 8, 5
    st = abi.empty_server_states(G, N)
    runs = _runs(16, length=2)
    t0, t1 = [], []
    for g in range(G):
        s = g * N
        x = 8 if g % 2 == 0 else 33
        _leader(st, s, N, runs, 32, 17, x)
        if g % 2:
            st["match_index"][s, 3] = x             # three members at 33: the agreed index is the appended entry
        ap = np.zeros(1, dtype=abi.MSG_DTYPE)
        ap["server"], ap["kind"], ap["from"], ap["n_entries"] = s, abi.MSG_APPEND, abi.NONE, 1
        t0.append(ap)
        t1.append(_reply(s, N, 1, 17, x))
        # the model: runs 1..15 and (33, 17) remain, first_index = 3; even groups agree on 8 (an old run: the gate is
        # foregone), odd groups on 33 (the new run of the current term: commit moves)
        after = runs[1:] + [(33, 17)]
        p = _agreed(st[s], N, 32, counted=(1, x))
        f = _facts(after, after[0][0], 33, 17, p)
        assert f["canonical"] and f["in_range"] and f["lrt_le_ct"] and p == x and (p < after[-2][0]) == (g % 2 == 0), f
    return st, [np.concatenate(t0), np.concatenate(t1)]


# ------------------------------------------------------------------------------------------------- the harness --
def _upload(buf, arr):
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    if buf.on_gpu:
        import torch
        buf.t[:raw.nbytes].copy_(torch.from_numpy(raw.copy()))
    else:
        buf.a[:raw.nbytes] = raw


def check_all_launch_forms(engine, oracle_lib, G, N, st0, ticks, on_gpu, want_flag=0):
    S, T = G * N, len(ticks)
    stride = max(len(m) for m in ticks)
    # bucket order (class, shard, success flag): what a train needs, and family order enough for the class kernel
    order = []
    bcs = np.zeros((T, engine.TRAIN_BUCKETS), dtype=np.uint32)
    kinds = np.zeros((T, abi.N_KINDS), dtype=np.uint32)
    host = np.zeros(T * stride, dtype=abi.MSG_DTYPE)
    h_st = np.zeros(T * stride, dtype=np.uint8)
    sent = np.zeros(S, dtype=np.uint8)
    for t, m in enumerate(ticks):
        assert len(np.unique(m["server"])) == len(m), "one message per server per tick"
        bk = engine.train_bucket(m["kind"], m["flags"], m["server"], N)
        m = m[np.argsort(bk, kind="stable")]
        order.append(m)
        bcs[t] = np.bincount(np.sort(bk), minlength=engine.TRAIN_BUCKETS)
        kinds[t] = np.bincount(m["kind"], minlength=abi.N_KINDS)
        host[t * stride:t * stride + len(m)] = m
        h_st[t * stride:t * stride + len(m)] = sent[m["server"]]
        sent[m["server"]] += 1
    counts = np.array([len(m) for m in order], dtype=np.uint32)
    # the oracle: set_state / get_state is the identity, then the ticks
    cpu = oracle_lib.Oracle(G, N, max_runs=16)
    cpu.set_state(0, st0)
    assert cpu.get_state().tobytes() == st0.tobytes(), "oracle: get_state after set_state"
    want = [cpu.step_parallel(m)[0] for m in order]
    want_state = cpu.get_state()
    want_sum = engine.combine_checksums(oracle_lib.server_checksums(want_state))
    cpu.close()
    if want_flag:
        assert all((w["flags"] & want_flag).all() for w in want[:1]), "the oracle reports the flag the case is about"
    moved = sum(int((w["flags"] & abi.F_AUX_EVAL != 0).sum()) for w in want)
    assert moved > 0, "some message of the stream moves commit_index"

    def decisions(buf, what):
        got = abi.expand_decisions(buf.host()[:T * stride * 64].view(abi.DECISION_DTYPE).copy())
        for t in range(T):
            g = got[t * stride:t * stride + len(order[t])]
            if g.tobytes() != want[t].tobytes():
                bad = int(np.flatnonzero((g.view(np.uint8).reshape(-1, 64) != want[t].view(np.uint8).reshape(-1, 64)).any(axis=1))[0])
                raise AssertionError(f"{what}: tick {t} message {bad}: {order[t][bad]}\n got    {g[bad]}\n oracle {want[t][bad]}")

    for flags, form in ((0, None), (abi.CFG_TRAIN_PERSISTENT, "persistent")):
        eng = engine.RaGpuBatch(G, N, max_runs=16, ring_slots=1, ring_capacity=64, flags=flags)
        d_msgs, d_stamps = Buf(T * stride * 64, on_gpu), Buf(T * stride, on_gpu)
        d_rpcs = Buf(T * stride * max(N - 1, 1) * 56, on_gpu)
        _upload(d_msgs, host)
        _upload(d_stamps, h_st)
        eng.set_state(0, st0)
        assert eng.get_state().tobytes() == st0.tobytes(), "engine: get_state after set_state"
        if form is None:
            # per-tick launches: the kind-generic kernel, then the class kernel
            for kc, what in ((None, "per-tick launch"), (kinds, "class kernel")):
                eng.set_state(0, st0)
                d_dec = Buf(T * stride * 64, on_gpu)
                eng.run_ticks_device(d_msgs.ptr, stride, T, d_dec.ptr, d_rpcs.ptr, tick_counts=counts, kind_counts=kc)
                eng.synchronize()
                decisions(d_dec, what)
                assert eng.get_state().tobytes() == want_state.tobytes(), what + ": state"
                assert eng.state_checksum() == want_sum, what + ": checksum"
            eng.set_state(0, st0)
        plan = eng.train_plan(bcs)
        d_dec = Buf(T * stride * 64, on_gpu)
        eng.train_run_device(plan, 0, T, d_msgs.ptr, d_stamps.ptr, stride, d_dec.ptr, d_rpcs.ptr, rpc_ring=T)
        eng.synchronize()
        assert eng.train_status()[0] == 0
        what = "train, " + eng.train_form()
        if form is not None:
            assert eng.train_form() == form
        elif on_gpu:
            assert eng.train_form() == "dealt", "the device deals its blocks round robin: the default form is the dealt kernel"
        decisions(d_dec, what)
        assert eng.get_state().tobytes() == want_state.tobytes(), what + ": state"
        assert eng.state_checksum() == want_sum, what + ": checksum"
        plan.close()
        eng.close()


@pytest.fixture(scope="module")
def scenarios():
    """Built once (and checked for coverage by the numpy model, before any engine exists); never modified."""
    out = {}
    for N in (5, 7):
        st, ticks, seen = _scenario(N)
        out[N] = (8, N, st, ticks, 0)
    st, ticks = _scenario_slice()
    out["slice"] = (264, 5, st, ticks, 0)
    st, ticks = _scenario_overflow()
    out["overflow"] = (8, 5, st, ticks, abi.F_RUNS_OVERFLOW)
    return out


KEYS = (5, 7, "slice", "overflow")


def _run(engine, oracle_lib, scenarios, key, on_gpu):
    G, N, st, ticks, flag = scenarios[key]
    check_all_launch_forms(engine, oracle_lib, G, N, st.copy(), [m.copy() for m in ticks], on_gpu, want_flag=flag)


@pytest.mark.parametrize("key", KEYS)
def test_quorum_gate_on_the_block_emulation(emulated_engine, oracle_lib, scenarios, key):
    _run(emulated_engine, oracle_lib, scenarios, key, False)


def test_range_below_the_oldest_run_is_refused(emulated_engine, oracle_lib):
    """The state the issue's case (e) names -- first_index below the oldest run's start -- cannot be uploaded: the
    canonical bit's clause "run 0 starts at or below first_index" holds for every table rgb_pack_kernel sees."""
    st = abi.empty_server_states(1, 5)
    _leader(st, 0, 5, _runs(3, first=10), 18, 3, 7, first=5, snapshot=(7, 3))
    cpu = oracle_lib.Oracle(1, 5, max_runs=16)
    with pytest.raises(ValueError):
        cpu.set_state(0, st)
    cpu.close()
    with emulated_engine.RaGpuBatch(1, 5, max_runs=16, ring_slots=1, ring_capacity=64) as eng:
        with pytest.raises(emulated_engine.RgbError):
            eng.set_state(0, st)


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_quorum_gate_on_the_gpu(oracle_lib, scenarios, key):
    from ra_amd import engine
    _run(engine, oracle_lib, scenarios, key, True)
