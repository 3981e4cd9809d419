"""The run a snapshot_written event cuts at, found by bisection on a canonical table (packed-word bit PK_CANON_SH,
run_search_canonical in rgb_kernels.hip; call sites: log_snapshot_written and truncate_runs_to through find_run<true>).

A snapshot_written message does nothing but log_snapshot_written: the run that holds index + 1 becomes run 0, the runs
behind it move to the front.  On a row whose table is canonical -- run starts and terms strictly increasing, run 0 at or
below first_index -- the in-memory runs are searched by halving; every other row walks them newest first as before.
Both must give what the oracle gives, whatever the table size and wherever the index falls.

States are built by hand.  For every table size n_runs in SIZES a snapshot_written is sent whose index + 1 is
  * the first index of run k and the last index of run k, for every k,
  * first_index itself (the index below the range: no effect) and first_index + 1 (the message names first_index),
  * last_index + 1 (the message names last_index: the range is emptied),
  * an index below first_index (no effect),
each on a row of its own (one snapshot_written per server: the state compared at the end of the stream IS the state after
that step, for every case; the per-tick launches are also compared with the oracle's whole state after every tick).
The cases of a table rotate through the five roles: the specialised kernels make one log_snapshot_written call for every
role together (process_message), the kind-generic kernel goes through each role's handler.
The same cases run on rows whose bit is clear, cleared two ways: an uploaded table whose terms are out of order (no
such table has one run), and a follower whose table of n_runs - 2 runs is given two runs of LOWER terms by an
append_entries_rpc one tick earlier (the push clears the bit; n_runs >= 3).  A last scenario sends one tick in which
every server gets the event, rows cycling through: canonical with index + 1 in run 0 (the walk of the whole table that
the bisection replaces), canonical found at the first probe, non-canonical, canonical in the middle -- every 64
consecutive messages of the tick (a slice of the per-tick kernels) and every train bucket hold all four.
Before any engine runs, the numpy model below checks that the cases are what they claim to be.  Expected decisions,
states and checksums come from the oracle alone; every stream runs through the kind-generic per-tick kernel, the
per-tick class kernel and a train launch in the default and in the persistent form."""
import numpy as np
import pytest

from ra_amd import abi
from test_train import Buf
from test_quorum_gate_canonical import _upload, _term_at

UNDEF = abi.UNDEF_INT
SIZES = (1, 2, 3, 4, 5, 10, 11, 16)
G = 64
FIRST, LEN = 10, 3


# ------------------------------------------------------------------------------------------------ state builders --
def _table(n, canonical=True):
    terms = list(range(1, n + 1))
    if not canonical:
        terms[0], terms[1] = terms[1], terms[0]           # starts still increase (an upload must), terms do not
    return [(FIRST + LEN * k, terms[k]) for k in range(n)]


def _is_canonical(runs, first):
    return runs[0][0] <= first and all(a[0] < b[0] and a[1] < b[1] for a, b in zip(runs, runs[1:]))


def _run_of(runs, idx):
    return max([k for k, (a, _) in enumerate(runs) if a <= idx], default=-1)


def _case_indexes(runs, li):
    """The snapshot indexes (index + 1 = what the list in the module docstring names), in order, without repeats."""
    first = runs[0][0]
    ends = [a for a, _ in runs[1:]] + [li + 1]
    nf = [a for a, _ in runs] + [e - 1 for e in ends] + [first, first + 1, li + 1, first - 2]
    out = []
    for x in nf:
        if x - 1 not in out:
            out.append(x - 1)
    return out


def _follower(st, s, N, runs, li, ct, lwi=None):
    r = st[s:s + 1]
    r["first_index"], r["last_index"], r["last_term"], r["n_runs"] = runs[0][0], li, runs[-1][1], len(runs)
    for k, (a, t) in enumerate(runs):
        st["run_start"][s, k], st["run_term"][s, k] = a, t
    lwi = li if lwi is None else lwi
    r["last_written_index"], r["last_written_term"], r["pending_first"] = lwi, _term_at(runs, lwi), lwi + 1
    r["current_term"] = ct
    r["commit_index"] = r["last_applied"] = li
    r["leader_id"] = (s % N + 1) % N                       # a known leader: a changed last_written is acknowledged


def _as_leader(st, s, N, li):
    me = s % N
    st["role"][s], st["leader_id"][s], st["voted_for"][s] = abi.ROLE_LEADER, me, me
    for j in range(N):
        st["next_index"][s, j] = li + 1
        st["match_index"][s, j] = 0 if j == me else li
        st["commit_index_sent"][s, j] = li


def _as_role(st, s, N, li, i):
    """Case i of a table runs in role i mod 5: the specialised kernels serve the event with ONE call for every role (a
    follower also acknowledges a last_written that moved), the kind-generic kernel through each role's handler."""
    me = s % N
    role = (abi.ROLE_FOLLOWER, abi.ROLE_LEADER, abi.ROLE_CANDIDATE, abi.ROLE_PRE_VOTE, abi.ROLE_AWAIT_CONDITION)[i % 5]
    if role == abi.ROLE_LEADER:
        _as_leader(st, s, N, li)
    elif role in (abi.ROLE_CANDIDATE, abi.ROLE_PRE_VOTE):
        st["role"][s], st["leader_id"][s] = role, abi.NONE
        if role == abi.ROLE_CANDIDATE:
            st["voted_for"][s], st["votes"][s] = me, 1
    elif role == abi.ROLE_AWAIT_CONDITION:
        st["role"][s] = role
    return role


def _snapshot_written(s, idx, term):
    m = np.zeros(1, dtype=abi.MSG_DTYPE)
    m["server"], m["kind"], m["from"], m["a"], m["b"] = s, abi.MSG_SNAPSHOT_WRITTEN, abi.NONE, idx, term
    return m


def _snap_term(runs, idx):
    t = _term_at(runs, idx)
    return 1 if t is None else t


# ------------------------------------------------------------------------------------------------------ scenarios --
def _scenario_uploaded(N):
    """64 groups x N, one tick: every case on a canonical row and on a row uploaded with its terms out of order."""
    st = abi.empty_server_states(G, N)
    msgs, s, seen, roles = [], 0, {}, set()
    for canonical in (True, False):
        for n in SIZES:
            if n == 1 and not canonical:
                continue                                   # one run is always canonical
            runs = _table(n, canonical)
            li = FIRST + LEN * n - 1
            assert _is_canonical(runs, FIRST) == canonical
            for i, idx in enumerate(_case_indexes(runs, li)):
                _follower(st, s, N, runs, li, ct=n + 5, lwi=FIRST if i % 3 == 1 else None)
                roles.add((canonical, _as_role(st, s, N, li, i + n)))
                msgs.append(_snapshot_written(s, idx, _snap_term(runs, idx)))
                k = _run_of(runs, idx + 1) if FIRST <= idx < li else None
                seen.setdefault((canonical, n), set()).add("none" if idx < FIRST else "emptied" if idx >= li else k)
                s += 1
    assert s <= G * N and len(roles) == 10, "every role on canonical and on non-canonical rows"
    for (canonical, n), got in seen.items():
        assert got == set(range(n)) | {"none", "emptied"}, (canonical, n, got)   # the cut falls in every run
    return st, [np.concatenate(msgs)]


def _scenario_rpc(N):
    """64 groups x N, two ticks: a canonical follower of n_runs - 2 runs is given two runs of lower terms by an
    append_entries_rpc, then the cases over the table of n_runs runs."""
    st = abi.empty_server_states(G, N)
    t0, t1, s = [], [], 0
    for n in (3, 4, 5, 10, 11, 16):
        base = [(FIRST + LEN * k, k + 1 if k < n - 3 else 90) for k in range(n - 2)]
        li0 = FIRST + LEN * (n - 2) - 1
        after = base + [(li0 + 1, 50), (li0 + 3, 60)]
        li = li0 + 4
        assert _is_canonical(base, FIRST) and not _is_canonical(after, FIRST) and len(after) == n
        assert all(a[0] < b[0] for a, b in zip(after, after[1:])) and after[-2][1] < base[-1][1]
        kinds = set()
        for idx in _case_indexes(after, li):
            _follower(st, s, N, base, li0, ct=100)
            aer = np.zeros(1, dtype=abi.MSG_DTYPE)
            aer["server"], aer["kind"], aer["from"], aer["term"] = s, abi.MSG_AER, (s % N + 1) % N, 100
            aer["a"], aer["b"], aer["c"] = li0, 90, li0
            aer["n_entries"], aer["n_run0"], aer["run0_term"], aer["run1_term"] = 4, 2, 50, 60
            t0.append(aer)
            t1.append(_snapshot_written(s, idx, _snap_term(after, idx)))
            kinds.add("none" if idx < FIRST else "emptied" if idx >= li else _run_of(after, idx + 1))
            s += 1
        assert kinds == set(range(n)) | {"none", "emptied"}, (n, kinds)
    assert s <= G * N
    return st, [np.concatenate(t0), np.concatenate(t1)]


def _scenario_mixed(N, engine):
    """64 groups x N, one tick, every server: 0 = canonical, index + 1 in run 0 of 16 (the whole-table walk); 1 =
    canonical, the newest in-memory run (found at once); 2 = terms out of order; 3 = canonical, run 4 of 11."""
    st = abi.empty_server_states(G, N)
    msgs, what = [], []
    for s in range(G * N):
        c = s % 4
        n = 11 if c == 3 else 16
        runs = _table(n, canonical=c != 2)
        li = FIRST + LEN * n - 1
        k = (0, n - 3, 5, 4)[c]
        idx = runs[k][0]                                   # index + 1 is the second index of run k
        assert _run_of(runs, idx + 1) == k and _is_canonical(runs, FIRST) == (c != 2)
        _follower(st, s, N, runs, li, ct=n + 5)
        if s % N == 0:
            _as_leader(st, s, N, li)                       # member 0 leads: every slice holds leaders and followers
        msgs.append(_snapshot_written(s, idx, runs[k][1]))
        what.append(c)
    m = np.concatenate(msgs)
    order = np.argsort(engine.train_bucket(m["kind"], m["flags"], m["server"], N), kind="stable")
    cls = np.array(what)[order]
    for i in range(0, len(cls) - 63):
        assert len(set(cls[i:i + 64])) == 4, "every 64 consecutive messages of the tick mix the four rows"
    for shard in range(8):
        assert len(set(np.array(what)[(m["server"] // N) % 8 == shard])) == 4
    return st, [m]


# ------------------------------------------------------------------------------------------------- the harness --
def check_all_launch_forms(engine, oracle_lib, N, st0, ticks, on_gpu):
    S, T = G * N, len(ticks)
    stride = max(len(m) for m in ticks)
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
    cpu = oracle_lib.Oracle(G, N, max_runs=16)
    cpu.set_state(0, st0)
    assert cpu.get_state().tobytes() == st0.tobytes(), "oracle: get_state after set_state"
    want, want_states = [], []
    for m in order:
        want.append(cpu.step_parallel(m)[0])
        want_states.append(cpu.get_state())
    want_sum = engine.combine_checksums(oracle_lib.server_checksums(want_states[-1]))
    cpu.close()
    assert not any(w["invariant"].any() for w in want), "no case trips an invariant"
    assert want_states[-1].tobytes() != st0.tobytes()

    def decisions(buf, what, t0, n):
        got = abi.expand_decisions(buf.host()[:T * stride * 64].view(abi.DECISION_DTYPE).copy())
        for t in range(t0, t0 + n):
            g = got[t * stride:t * stride + len(order[t])]
            if g.tobytes() != want[t].tobytes():
                bad = int(np.flatnonzero((g.view(np.uint8).reshape(-1, 64) != want[t].view(np.uint8).reshape(-1, 64)).any(axis=1))[0])
                raise AssertionError(f"{what}: tick {t} message {bad}: {order[t][bad]}\n got    {g[bad]}\n oracle {want[t][bad]}")

    def state(eng, what, t):
        got = eng.get_state()
        if got.tobytes() != want_states[t].tobytes():
            bad = int(np.flatnonzero((got.view(np.uint8).reshape(S, -1) != want_states[t].view(np.uint8).reshape(S, -1)).any(axis=1))[0])
            raise AssertionError(f"{what}: state after tick {t}, server {bad}:\n got    {got[bad]}\n oracle {want_states[t][bad]}")

    for flags, form in ((0, None), (abi.CFG_TRAIN_PERSISTENT, "persistent")):
        eng = engine.RaGpuBatch(G, N, max_runs=16, ring_slots=1, ring_capacity=64, flags=flags)
        d_msgs, d_stamps = Buf(T * stride * 64, on_gpu), Buf(T * stride, on_gpu)
        d_rpcs = Buf(T * stride * max(N - 1, 1) * 56, on_gpu)
        _upload(d_msgs, host)
        _upload(d_stamps, h_st)
        if form is None:
            for kc, what in ((None, "per-tick launch"), (kinds, "class kernel")):
                eng.set_state(0, st0)
                d_dec = Buf(T * stride * 64, on_gpu)
                for t in range(T):                                  # tick by tick: the whole state after every step
                    eng.run_ticks_device(d_msgs.ptr + t * stride * 64, stride, 1, d_dec.ptr + t * stride * 64, d_rpcs.ptr,
                                         tick_counts=counts[t:t + 1], kind_counts=None if kc is None else kc[t:t + 1])
                    eng.synchronize()
                    decisions(d_dec, what, t, 1)
                    state(eng, what, t)
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
            assert eng.train_form() == "dealt"
        decisions(d_dec, what, 0, T)
        state(eng, what, T - 1)
        assert eng.state_checksum() == want_sum, what + ": checksum"
        plan.close()
        eng.close()


@pytest.fixture(scope="module")
def scenarios():
    """Built once, checked by the numpy model before any engine exists, never modified."""
    from ra_amd import engine
    out = {}
    for N in (5, 7):
        out["uploaded", N] = _scenario_uploaded(N)
        out["rpc", N] = _scenario_rpc(N)
        out["mixed", N] = _scenario_mixed(N, engine)
    return out


KEYS = [(k, N) for k in ("uploaded", "rpc", "mixed") for N in (5, 7)]


def _run(engine, oracle_lib, scenarios, key, on_gpu):
    st, ticks = scenarios[key]
    assert len(ticks) <= 8
    check_all_launch_forms(engine, oracle_lib, key[1], st.copy(), [m.copy() for m in ticks], on_gpu)


@pytest.mark.parametrize("key", KEYS, ids=lambda k: f"{k[0]}-{k[1]}")
def test_snapshot_written_cut_on_the_block_emulation(emulated_engine, oracle_lib, scenarios, key):
    _run(emulated_engine, oracle_lib, scenarios, key, False)


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS, ids=lambda k: f"{k[0]}-{k[1]}")
def test_snapshot_written_cut_on_the_gpu(oracle_lib, scenarios, key):
    from ra_amd import engine
    _run(engine, oracle_lib, scenarios, key, True)
