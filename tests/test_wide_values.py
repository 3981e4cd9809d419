"""Full-width values on the Raft path.  The ABI's indexes and terms are uint64_t, "the reference's integers"
(include/ra_gpu_batch.h), and the differential fuzz draws them within a few hundred of zero: a compare done as signed,
a 32-bit intermediate or a token compared on one of its words would not show.  Here the same random states and ticks
run with every index and term shifted (fuzz.widen) so that they sit below, across and above 2^32, at 2^53 and across
2^63, with 64-bit pre-vote tokens and machine versions over the whole u32 range.  Every check is bit-exact against the
CPU checker; there is no tolerance.

Contract: every value stays below RGB_UNDEF - 2^16 (fuzz.WIDE_LIMIT).  The sentinel's neighbourhood is outside the
contract -- RGB_UNDEF is `undefined`, not an index, and the clause code may form index + n for the n of one message.

Every check is a plain function of an engine module: once on the emulated library, once (`-m gpu`) on the device."""
import os

import numpy as np
import pytest

import fuzz
from ra_amd import abi
from test_compact_decisions import Buf, assert_state_equal, in_bucket_order, rpc_slots
from test_fused_pipeline import check_fused
from test_gpu_parity import check_quorum_term_gate, quorum_gate_states


@pytest.fixture(scope="module")
def gpu_engine():
    from ra_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build()    # a fresh checkout on the GPU box: hipcc is there, the .so is not in git
    engine.lib()          # raises if the HIP library is missing: no fallback
    return engine


# (index offset, term offset)
OFFSETS = [(2**32 - 20, 0),               # the indexes cross 2^32 during the run
           (0, 2**32 - 3),                # the terms do
           (2**32 + 7, 2**32 + 5),
           (2**53 - 9, 2**40),            # where a double stops counting
           (2**63 - 30, 2**63 - 4)]       # both cross the sign bit
IDS = ["index_across_2p32", "term_across_2p32", "above_2p32", "2p53", "across_2p63"]
# groups for N members: whole wavefronts and a ragged tail; the emulated twins run half of that
GROUPS = {1: 300, 3: 130, 5: 130, 7: 80, 8: 70}


def groups_for(n_members, on_gpu):
    return GROUPS[n_members] if on_gpu else GROUPS[n_members] // 2


def wide_states(seed, G, N, offsets, rng=None):
    rng = np.random.default_rng(seed) if rng is None else rng
    return fuzz.widen(fuzz.random_states(rng, G, N, max_runs=6), N, offsets[0], offsets[1], rng)


# ------------------------------------------------------------------------------------------ identity

# (rgb_upload_state ties last_term and the run starts to their neighbours: those move with the whole state above)
HIGH_WORD_FIELDS = ["current_term", "commit_index", "last_applied", "last_written_index", "last_written_term",
                    "pending_first", "pre_vote_token", "query_index", ("run_term", 0), ("run_term", 1)]
PEER_FIELDS = ["match_index", "next_index", "commit_index_sent", "peer_query_index"]


def check_identity(engine, O, N, G, offsets):
    """rgb_upload_state / rgb_download_state hand every word back, and rgb_state_checksum (= the checker's, word for
    word) sees the high word of every field."""
    st = wide_states(41, G, N, offsets)
    cpu = O.Oracle(G, N)
    cpu.set_state(0, st)
    canon = cpu.get_state()                     # the canonical form of the same state (unused slots cleared)
    with engine.RaGpuBatch(G, N, max_runs=16, ring_slots=1, ring_capacity=64) as eng:
        eng.set_state(0, st)
        got = eng.get_state()
        assert_state_equal("upload / download", got, canon)
        for f in ("current_term", "commit_index", "last_applied", "last_index", "last_term", "last_written_index",
                  "last_written_term", "first_index", "pending_first", "pre_vote_token", "query_index", "machine_version",
                  "effective_machine_version", "match_index", "next_index", "commit_index_sent"):
            assert np.array_equal(got[f], st[f]), f"{f} does not come back as it went in"
        assert eng.state_checksum() == engine.combine_checksums(O.server_checksums(canon))
        # one high word changed in one server: the checksum of that server moves, and moves as the checker's does
        s = next(i for i in range(len(st)) if int(st["n_runs"][i]) >= 3 and int(st["role"][i]) == abi.ROLE_LEADER)
        base = eng.state_checksum(s, 1)
        peer = (int(st["self"][s]) + 1) % N
        for f in HIGH_WORD_FIELDS + ([(p, peer) for p in PEER_FIELDS] if N > 1 else []):
            for bit in (32, 47, 63):
                one = canon[s:s + 1].copy()
                if isinstance(f, tuple):
                    one[f[0]][0, f[1]] ^= np.uint64(1 << bit)
                else:
                    one[f][0] ^= np.uint64(1 << bit)
                eng.set_state(s, one)
                now = eng.state_checksum(s, 1)
                assert now != base, f"bit {bit} of {f} does not reach the state checksum"
        eng.set_state(s, canon[s:s + 1])
        assert eng.state_checksum(s, 1) == base
    cpu.close()


# ------------------------------------------------------------------------------------------ random ticks

def checker_ticks(O, st, G, N, rng, n_ticks, max_runs, engine=None, partner=False):
    """n_ticks of fuzz.random_msgs applied by the checker: [(msgs, decisions, rpcs, state after)].  engine: the ticks
    are put in bucket order (what the device-resident entry points want).  partner: every other tick derives a server's
    message from the row of its NEIGHBOUR in the group (one-sided groups: the message's values lie 2^32 .. 2^63 away
    from the server's own)."""
    cpu = O.Oracle(G, N, max_runs=max_runs)
    cpu.set_state(0, st)
    out = []
    idx = np.arange(G * N)
    neighbour = (idx // N) * N + (idx % N + 1) % N
    for t in range(n_ticks):
        cur = cpu.get_state()
        msgs = fuzz.random_msgs(rng, cur[neighbour] if partner and t % 2 == 0 else cur, N, wide=True)
        if engine is not None:                  # (the class kernels and the trains take no NOP records)
            msgs = in_bucket_order(engine, msgs[msgs["kind"] != abi.MSG_NOP], N)
        d, r = cpu.step(msgs)
        out.append((msgs, d, r.copy(), cpu.get_state()))
    cpu.close()
    return out


def first_difference(tag, msgs, got, want):
    bad = np.flatnonzero((got.view(np.uint8).reshape(-1, 64) != want.view(np.uint8).reshape(-1, 64)).any(axis=1))
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{tag}: decision {i} of {len(bad)} that differ: msg={msgs[i]}\n got ={got[i]}\n want={want[i]}")


def run_host_path(engine, O, tag, st, G, N, ticks, max_runs):
    with engine.RaGpuBatch(G, N, max_runs=max_runs, ring_slots=2, ring_capacity=max(1024, G * N)) as eng:
        eng.set_state(0, st)
        for t, (msgs, want_d, want_r, want_s) in enumerate(ticks):
            dg, rg = eng.step(msgs)
            assert len(dg) == len(want_d)
            first_difference(f"{tag}, rgb_submit, tick {t}", msgs, dg, want_d)
            assert fuzz.sort_rpcs(rg.copy()).tobytes() == fuzz.sort_rpcs(want_r).tobytes(), f"{tag}, rgb_submit, tick {t}: rpc records"
            assert_state_equal(f"{tag}, rgb_submit, tick {t}", eng.get_state(), want_s)
        assert eng.state_checksum() == engine.combine_checksums(O.server_checksums(ticks[-1][3]))


def run_device_paths(engine, tag, st, G, N, ticks, max_runs, on_gpu):
    """The bucket-ordered ticks through rgb_run_ticks_device (kind-generic, class kernels) and one train launch."""
    S, T, per = G * N, len(ticks), max(N - 1, 1)
    tb, rs = S * 64, S * per * 56
    counts = np.array([len(t[0]) for t in ticks], dtype=np.uint32)
    kinds = np.array([np.bincount(t[0]["kind"], minlength=abi.N_KINDS) for t in ticks], dtype=np.uint32)
    buckets = np.array([np.bincount(engine.train_bucket(t[0]["kind"], t[0]["flags"], t[0]["server"], N),
                                    minlength=engine.TRAIN_BUCKETS) for t in ticks], dtype=np.uint32)
    dmsgs = Buf(T * tb, on_gpu)
    for t in range(T):
        dmsgs.put(t * tb, ticks[t][0].tobytes())

    def want_rpcs(t):
        r = fuzz.sort_rpcs(ticks[t][2]).copy()
        r["msg_index"] = 0
        return r

    def decisions(buf, t, at):
        return abi.expand_decisions(buf.host()[at * tb:at * tb + int(counts[t]) * 64].view(abi.DECISION_DTYPE))

    with engine.RaGpuBatch(G, N, max_runs=max_runs, ring_slots=1, ring_capacity=64) as eng:
        for name, kc in (("generic kernel", None), ("class kernels", kinds)):
            eng.set_state(0, st)
            for t in range(T):
                ddec, drpc = Buf(tb, on_gpu), Buf(rs, on_gpu)
                eng.run_ticks_device(dmsgs.ptr + t * tb, S, 1, ddec.ptr, drpc.ptr, tick_counts=counts[t:t + 1],
                                     kind_counts=None if kc is None else kc[t:t + 1])
                eng.synchronize()
                first_difference(f"{tag}, {name}, tick {t}", ticks[t][0], decisions(ddec, t, 0), ticks[t][1])
                assert rpc_slots(drpc.host()[:rs], ticks[t][1], per).tobytes() == want_rpcs(t).tobytes(), f"{tag}, {name}, tick {t}: rpc records"
                assert_state_equal(f"{tag}, {name}, tick {t}", eng.get_state(), ticks[t][3])
        eng.set_state(0, st)
        plan = eng.train_plan(buckets)
        stamps, ddec, drpc = Buf(T * S, on_gpu), Buf(T * tb, on_gpu), Buf(T * rs, on_gpu)
        eng.train_stamp_device(dmsgs.ptr, stamps.ptr, S, counts)
        eng.train_run_device(plan, 0, T, dmsgs.ptr, stamps.ptr, S, ddec.ptr, drpc.ptr, rpc_ring=T)
        eng.synchronize()
        assert eng.train_status()[0] == 0
        for t in range(T):
            first_difference(f"{tag}, train, tick {t}", ticks[t][0], decisions(ddec, t, t), ticks[t][1])
            assert rpc_slots(drpc.host()[t * rs:(t + 1) * rs], ticks[t][1], per).tobytes() == want_rpcs(t).tobytes(), f"{tag}, train, tick {t}: rpc records"
        assert_state_equal(f"{tag}, train", eng.get_state(), ticks[-1][3])
        plan.close()


def check_random_ticks(engine, O, N, offsets, max_runs, on_gpu, seed, n_ticks=5):
    G = groups_for(N, on_gpu)
    tag = f"N={N} G={G} max_runs={max_runs} offsets=({offsets[0]:#x}, {offsets[1]:#x})"
    rng = np.random.default_rng(seed)
    st = wide_states(seed, G, N, offsets, rng)
    ticks = checker_ticks(O, st, G, N, rng, n_ticks, max_runs, engine)
    if max_runs < 6:
        assert any(((t[1]["flags"] & abi.F_RUNS_OVERFLOW) != 0).any() for t in ticks), f"{tag}: the run table never overflowed"
    run_host_path(engine, O, tag, st, G, N, ticks, max_runs)
    run_device_paths(engine, tag, st, G, N, ticks, max_runs, on_gpu)


# every offset pair with every group size and both run-table sizes at least once
TICK_CASES = [(5, 0, 16), (5, 1, 4), (5, 2, 16), (5, 3, 4), (5, 4, 16), (5, 4, 4), (1, 0, 4), (1, 4, 16), (3, 1, 16), (3, 4, 4),
              (7, 2, 4), (7, 4, 16), (8, 3, 16), (8, 4, 4), (8, 0, 16)]


def _tick_id(c):
    return f"N{c[0]}-{IDS[c[1]]}-runs{c[2]}"


# ------------------------------------------------------------------------------------------ quorum

def check_quorum(engine, O, groups, built, offsets, seed):
    """The cases of test_quorum_term_gate_on_any_run_table (tests/test_gpu_parity.py) on widened states: the sorting
    network and the term gate compare values that straddle 2^32 / 2^63 inside one server's list."""
    rng = np.random.default_rng(seed)
    N = 5
    st = fuzz.widen(quorum_gate_states(rng, built, N), N, *offsets)
    lo, hi = int(st["match_index"][:, :N].min()), int(st["match_index"][:, :N].max())
    for edge in (2**32, 2**63):
        if offsets[0] < edge <= offsets[0] + 30:
            assert lo < edge <= hi, "the match indexes do not straddle the edge"
    st = np.tile(st, groups // built)
    check_quorum_term_gate(engine, O, st, groups, N, rng)


QUORUM_OFFSETS = [0, 1, 4]


# ------------------------------------------------------------------------------------------ leaderboard

def leaderboard_ref(st, G, N):
    """The row rule of include/ra_gpu_batch.h (rgb_leaderboard_row): the leader with the highest term (the lowest slot
    among equals), else the maximum over the members."""
    rows = np.zeros(G, dtype=abi.LEADERBOARD_DTYPE)
    for g in range(G):
        m = st[g * N:(g + 1) * N]
        lead = np.flatnonzero(m["role"] == abi.ROLE_LEADER)
        rows["n_leaders"][g], rows["term"][g] = len(lead), m["current_term"].max()
        if len(lead):
            l = lead[np.argmax(m["current_term"][lead])]
            rows["leader"][g], rows["commit_index"][g], rows["last_applied"][g] = l, m["commit_index"][l], m["last_applied"][l]
        else:
            rows["leader"][g], rows["commit_index"][g], rows["last_applied"][g] = abi.NONE, m["commit_index"].max(), m["last_applied"].max()
    return rows


def one_sided(st, wide, G, N, rng):
    """Groups in which some members are widened and the others are not: rows of `st` mixed back into `wide`."""
    mixed = wide.copy()
    keep = rng.random(G * N) < 0.4
    keep[::N] = np.arange(G) % 2 == 0          # slot 0 alternates, so every second group straddles for certain
    keep[1::N] = np.arange(G) % 2 == 1 if N > 1 else keep[1::N]
    mixed[keep] = st[keep]
    return mixed


def check_leaderboard(engine, N, G, offsets, seed):
    rng = np.random.default_rng(seed)
    st = fuzz.random_states(rng, G, N, max_runs=6)
    wide = fuzz.widen(st, N, offsets[0], offsets[1], rng)
    with engine.RaGpuBatch(G, N, max_runs=16, ring_slots=1, ring_capacity=64) as eng:
        for name, s in (("widened", wide), ("one-sided", one_sided(st, wide, G, N, rng))):
            # more leaders than the draw gives, and groups without one
            s = s.copy()
            s["role"][rng.random(G * N) < 0.25] = abi.ROLE_LEADER
            s["role"][:N * (G // 5)] = abi.ROLE_FOLLOWER
            eng.set_state(0, s)
            got, want = eng.snapshot(), leaderboard_ref(s, G, N)
            assert int((want["n_leaders"] > 1).sum()) > 0 or N == 1
            assert int((want["n_leaders"] == 0).sum()) > 0
            if name == "one-sided" and N > 1 and offsets[1]:
                terms = s["current_term"].reshape(G, N)
                assert int(((terms.min(axis=1) < offsets[1]) & (terms.max(axis=1) >= offsets[1])).sum()) > G // 4
            for g in np.flatnonzero([got[g].tobytes() != want[g].tobytes() for g in range(G)])[:1]:
                raise AssertionError(f"{name}, group {g}: snapshot row {got[g]} != {want[g]}\n terms {s['current_term'][g * N:(g + 1) * N]} "
                                     f"roles {s['role'][g * N:(g + 1) * N]}")


# ------------------------------------------------------------------------------------------ one-sided groups

def check_one_sided(engine, O, N, offsets, on_gpu, seed, n_ticks=4):
    """Members of one group 2^32 .. 2^63 apart, and messages derived from the neighbour's row: every subtraction of the
    clause code and every range test of compact_decision sees a huge unsigned difference.  Such a group is not a Raft
    group; the checker is the referee."""
    G = groups_for(N, on_gpu)
    tag = f"one-sided N={N} G={G} offsets=({offsets[0]:#x}, {offsets[1]:#x})"
    rng = np.random.default_rng(seed)
    st = fuzz.random_states(rng, G, N, max_runs=6)
    mixed = one_sided(st, fuzz.widen(st, N, offsets[0], offsets[1], rng), G, N, rng)
    ticks = checker_ticks(O, mixed, G, N, rng, n_ticks, 16, engine, partner=True)
    run_host_path(engine, O, tag, mixed, G, N, ticks, 16)
    run_device_paths(engine, tag, mixed, G, N, ticks, 16, on_gpu)


ONE_SIDED_CASES = [(5, 0), (3, 2), (8, 4), (5, 4)]


# ------------------------------------------------------------------------------------------ the twins

@pytest.mark.parametrize("n_members,k", [(5, 0), (1, 3), (8, 4)], ids=lambda v: str(v))
def test_identity_on_the_block_emulation(emulated_engine, oracle_lib, n_members, k):
    check_identity(emulated_engine, oracle_lib, n_members, 24, OFFSETS[k])


@pytest.mark.gpu
@pytest.mark.parametrize("n_members,k", [(5, 0), (1, 3), (8, 4), (3, 2), (7, 1)], ids=lambda v: str(v))
def test_gpu_identity(gpu_engine, oracle_lib, n_members, k):
    check_identity(gpu_engine, oracle_lib, n_members, 70, OFFSETS[k])


@pytest.mark.parametrize("case", TICK_CASES, ids=_tick_id)
def test_random_ticks_on_the_block_emulation(emulated_engine, oracle_lib, case):
    check_random_ticks(emulated_engine, oracle_lib, case[0], OFFSETS[case[1]], case[2], False, 500 + TICK_CASES.index(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", TICK_CASES, ids=_tick_id)
def test_gpu_random_ticks(gpu_engine, oracle_lib, case):
    check_random_ticks(gpu_engine, oracle_lib, case[0], OFFSETS[case[1]], case[2], True, 500 + TICK_CASES.index(case))


def test_fused_pipeline_on_wide_values_on_the_block_emulation(emulated_engine, oracle_lib):
    check_fused(emulated_engine, oracle_lib, 5, 65, 921, offsets=OFFSETS[4])


@pytest.mark.gpu
def test_gpu_fused_pipeline_on_wide_values(gpu_engine, oracle_lib):
    check_fused(gpu_engine, oracle_lib, 5, 130, 921, offsets=OFFSETS[4])
    check_fused(gpu_engine, oracle_lib, 8, 70, 922, offsets=OFFSETS[0])


@pytest.mark.parametrize("k", QUORUM_OFFSETS, ids=[IDS[k] for k in QUORUM_OFFSETS])
def test_quorum_on_the_block_emulation(emulated_engine, oracle_lib, k):
    check_quorum(emulated_engine, oracle_lib, 64, 64, OFFSETS[k], 240 + k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", QUORUM_OFFSETS, ids=[IDS[k] for k in QUORUM_OFFSETS])
def test_gpu_quorum(gpu_engine, oracle_lib, k):
    check_quorum(gpu_engine, oracle_lib, 64, 64, OFFSETS[k], 240 + k)              # the kind-generic kernel
    check_quorum(gpu_engine, oracle_lib, 4200, 420, OFFSETS[k], 250 + k)           # the class-dispatch kernel (>= 4096 messages)


@pytest.mark.parametrize("n_members,k", [(5, 4), (3, 1), (8, 2), (1, 4)], ids=lambda v: str(v))
def test_leaderboard_on_the_block_emulation(emulated_engine, n_members, k):
    check_leaderboard(emulated_engine, n_members, 65, OFFSETS[k], 260 + k)


@pytest.mark.gpu
@pytest.mark.parametrize("n_members,k", [(5, 4), (3, 1), (8, 2), (1, 4), (7, 3)], ids=lambda v: str(v))
def test_gpu_leaderboard(gpu_engine, n_members, k):
    check_leaderboard(gpu_engine, n_members, 130, OFFSETS[k], 260 + k)


@pytest.mark.parametrize("n_members,k", ONE_SIDED_CASES, ids=lambda v: str(v))
def test_one_sided_groups_on_the_block_emulation(emulated_engine, oracle_lib, n_members, k):
    check_one_sided(emulated_engine, oracle_lib, n_members, OFFSETS[k], False, 280 + k)


@pytest.mark.gpu
@pytest.mark.parametrize("n_members,k", ONE_SIDED_CASES, ids=lambda v: str(v))
def test_gpu_one_sided_groups(gpu_engine, oracle_lib, n_members, k):
    check_one_sided(gpu_engine, oracle_lib, n_members, OFFSETS[k], True, 280 + k)
