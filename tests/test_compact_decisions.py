"""Compact decisions (include/ra_gpu_batch.h, "Compact decisions"): the 32-byte form a device-resident decision stream
uses where a decision's values lie close together.

A1 pins the codec: compact_ref() below is the encoder written from the header's comment alone; a table of full records
holds both sides of every threshold of every form, at small values, around 2^32 and around 2^63; abi.expand_decisions
and rgb_decision_expand (a stand-alone C program under AddressSanitizer + UBSan) must give every record back.

A2 pins the device's encoder, its ballot-indexed store and the device's own decoder: states and messages are built so
that the CHECKER's decisions land on the rows of A1 (coverage is asserted from the checker's decisions alone, before an
engine is touched), the same ticks then run through rgb_run_ticks_device (kind-generic and class kernels), a train
launch, rgb_submit and rgb_submit_raw.  Every check is a plain function of an engine module: once on the emulated
library, once (`-m gpu`) on the device.

Layout of the pattern tick.  All its 512 records are written events to followers, 64 per shard (group mod 8), in shard
order, so a 64-record slice is the same whether a kernel cuts the tick from its start (rgb_run_ticks_device) or bucket
by bucket (trains).  Shard k holds pattern k of SLICE_PATTERNS: all compact, none, alternating, one full record at lane
0 / 31 / 32 / 63, one compact record among full ones.

Rows of A1 that no state reaches through the ABI (they stay with A1):
  confirmed  next is 0          reply_next_index is last_index + 1; last_index = RGB_UNDEF is outside the contract
  wrote      fst > lst, la > lst  an append_entries_rpc writes at least one entry, and one below last_applied is
                                RGB_INV_WRITE_BELOW_APPLIED (flag RGB_F_INVARIANT: another shape)
  wrote      w2 / w5 non-zero   a decision without a reply carries no reply term
  counted    w2 .. w5 non-zero  the same
  every form invariant / heartbeat_to / cancel_backoff on their own: each comes with a flag outside the plain set
             (RGB_F_INVARIANT, RGB_F_SEND_HEARTBEATS, RGB_F_CANCEL_SNAPSHOT_RETRY); RGB_F_COMPACT is never an input
Rows reached only from states a running server never holds, uploaded as they are (the checker is the referee, not Raft
safety): last > A (last_written_index above last_index), lterm > term (a written entry of a term above current_term),
d4 = 0 and la = A + 2 (last_applied at and above last_index + 1)."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from ra_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu_engine():
    from ra_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build()    # a fresh checkout on the GPU box: hipcc is there, the .so is not in git
    engine.lib()          # raises if the HIP library is missing: no fallback
    return engine


# ------------------------------------------------------------------------------------------ the encoder, from the header

PLAIN = abi.F_LEADER_MSG | abi.F_APPLIED | abi.F_AUX_EVAL | abi.F_PIPELINE       # flags that carry no words
CONFIRMED = abi.F_REPLY | abi.F_REPLY_SUCCESS
WORDS = ("reply_term", "reply_next_index", "reply_last_index", "reply_last_term", "commit_index", "last_applied")


def shape_of(r):
    """'counted' | 'wrote' | 'confirmed' | None from kind and flags, as the header tells the forms apart."""
    kind, shape = int(r["kind"]), int(r["flags"]) & ~PLAIN & ~abi.F_COMPACT
    if shape == 0 and kind in (abi.MSG_AER_REPLY, abi.MSG_WRITTEN):
        return "counted"
    if shape == abi.F_WROTE and kind == abi.MSG_AER:
        return "wrote"
    if shape == CONFIRMED and kind in (abi.MSG_AER, abi.MSG_WRITTEN):
        return "confirmed"
    return None


def deltas(r):
    """The differences the header's forms store, in the integers (Python's), keyed by the names of the rows."""
    term, nxt, last, lterm, ci, la = (int(r[f]) for f in WORDS)
    A = nxt - 1
    return {"d1": A - last, "d2": term - lterm, "d3": ci + 512 - A, "d4": A + 1 - la,
            "span": last - nxt, "lag": last - la}


LIMITS = {"d1": 0xFF, "d2": 0xF, "d3": 0x3FF, "d4": 0x3FF, "span": 0xFFFF, "lag": 0xFFFF}
FORM_DELTAS = {"confirmed": ("d1", "d2", "d3", "d4"), "wrote": ("span", "lag"), "counted": ()}


def compact_ref(r):
    """The 32 bytes the header describes for the full record r (one abi.DECISION_DTYPE record), or None when r is
    written in full."""
    flags = int(r["flags"])
    if int(r["invariant"]) or int(r["heartbeat_to"]) or int(r["cancel_backoff"]) or flags & abi.F_COMPACT:
        return None
    form = shape_of(r)
    term, nxt, last, lterm, ci, la = (int(r[f]) for f in WORDS)
    d = deltas(r)
    if form is None or any(not 0 <= d[k] <= LIMITS[k] for k in FORM_DELTAS[form]):
        return None
    if form == "counted":
        if term or nxt or last or lterm:
            return None
        aux, A, B = 0, ci, la
    elif form == "wrote":
        if term or lterm:
            return None
        aux, A, B = d["span"] | d["lag"] << 16, last, ci
    else:
        if nxt == 0:
            return None
        aux, A, B = d["d1"] | d["d2"] << 8 | d["d3"] << 12 | d["d4"] << 22, nxt - 1, term
    return r.tobytes()[:8] + struct.pack("<IIQQ", flags | abi.F_COMPACT, aux, A, B)


def rows_of(r):
    """The rows of the A1 table a full record lands on.  A threshold row ('confirmed d1=256') counts only when every
    other difference of the form fits: the named one alone decides."""
    form = shape_of(r)
    if form is None or int(r["invariant"]) or int(r["heartbeat_to"]) or int(r["cancel_backoff"]):
        base = r.copy()
        base["flags"] = int(r["flags"]) & (PLAIN | CONFIRMED | abi.F_WROTE)
        f = shape_of(base)
        return {f + " flag outside the plain set"} if form is None and f is not None and compact_ref(base) else set()
    out, d = set(), deltas(r)
    if form == "counted":
        return {"counted fits"} if compact_ref(r) else set()
    for k in FORM_DELTAS[form]:
        if all(0 <= d[o] <= LIMITS[o] for o in FORM_DELTAS[form] if o != k):
            for v in (0, LIMITS[k], LIMITS[k] + 1, -1):
                if d[k] == v:
                    out.add(f"{form} {k}={v}")
    return out


def record(kind, flags, words, server=7, role=abi.ROLE_FOLLOWER, reply_to=2, **kw):
    r = np.zeros(1, dtype=abi.DECISION_DTYPE)
    r["server"], r["role"], r["reply_to"], r["kind"], r["flags"] = server, role, reply_to, kind, flags
    for f, v in zip(WORDS, words):
        r[f] = v
    for f, v in kw.items():
        r[f] = v
    return r[0]


def confirmed(A, T, d1=3, d2=1, d3=510, d4=5, kind=abi.MSG_WRITTEN, flags=CONFIRMED, **kw):
    return record(kind, flags, (T, A + 1, A - d1, T - d2, A + d3 - 512, A + 1 - d4), **kw)


def wrote(A, T, span=2, lag=9, flags=abi.F_WROTE | abi.F_LEADER_MSG, w2=0, w5=0, **kw):
    return record(abi.MSG_AER, flags, (w2, A - span, A, w5, A - 4, A - lag), reply_to=abi.NONE, **kw)


def counted(A, T, kind=abi.MSG_AER_REPLY, flags=abi.F_APPLIED, words=(0, 0, 0, 0), **kw):
    return record(kind, flags, tuple(words) + (A, A - 3), role=abi.ROLE_LEADER, reply_to=abi.NONE, **kw)


BASES = [("small", 70_000, 20), ("around 2^32", 2**32 + 100, 2**32 + 3), ("around 2^63", 2**63 + 100, 2**63 + 3)]


def codec_table(A, T):
    """(row, full record, fits) -- both sides of every threshold of every form."""
    t = []
    for k, lim in (("d1", 0xFF), ("d2", 0xF), ("d3", 0x3FF), ("d4", 0x3FF)):
        t += [(f"confirmed {k}={lim}", confirmed(A, T, **{k: lim}), True),
              (f"confirmed {k}={lim + 1}", confirmed(A, T, **{k: lim + 1}), False)]
    t += [("confirmed d3=0", confirmed(A, T, d3=0), True), ("confirmed d3=-1", confirmed(A, T, d3=-1), False),
          ("confirmed d4=0", confirmed(A, T, d4=0), True), ("confirmed d4=-1", confirmed(A, T, d4=-1), False),
          ("confirmed d1=0", confirmed(A, T, d1=0), True), ("confirmed d1=-1", confirmed(A, T, d1=-1), False),
          ("confirmed d2=0", confirmed(A, T, d2=0), True), ("confirmed d2=-1", confirmed(A, T, d2=-1), False),
          ("confirmed every field at its limit", confirmed(A, T, d1=0xFF, d2=0xF, d3=0x3FF, d4=0x3FF, kind=abi.MSG_AER,
                                                           flags=CONFIRMED | PLAIN), True),
          ("confirmed next is 0", record(abi.MSG_WRITTEN, CONFIRMED, (T, 0, 0, T, 0, 0)), False),
          # .. and with every other word where arithmetic modulo 2^64 would make the differences fit
          ("confirmed next is 0, the rest wrapped", record(abi.MSG_WRITTEN, CONFIRMED, (T, 0, 2**64 - 4, T - 1, 2**64 - 3, 2**64 - 5)), False)]
    for k in ("span", "lag"):
        t += [(f"wrote {k}=65535", wrote(A, T, **{k: 0xFFFF}), True), (f"wrote {k}=65536", wrote(A, T, **{k: 0x10000}), False),
              (f"wrote {k}=0", wrote(A, T, **{k: 0}), True), (f"wrote {k}=-1", wrote(A, T, **{k: -1}), False)]
    t += [("wrote both at their limit", wrote(A, T, span=0xFFFF, lag=0xFFFF, flags=abi.F_WROTE | PLAIN), True),
          ("wrote w2", wrote(A, T, w2=T), False), ("wrote w5", wrote(A, T, w5=1), False)]
    t += [("counted fits", counted(A, T), True), ("counted written", counted(A, T, kind=abi.MSG_WRITTEN, flags=0), True),
          ("counted every plain flag", counted(A, T, flags=PLAIN), True)]
    for k in range(4):
        words = [0, 0, 0, 0]
        words[k] = 1 if k else T
        t.append((f"counted w{k + 2}", counted(A, T, words=words), False))
    # every form: each disqualifier on its own
    for form, make, own in (("confirmed", confirmed, CONFIRMED), ("wrote", wrote, abi.F_WROTE), ("counted", counted, 0)):
        t += [(f"{form} invariant", make(A, T, invariant=abi.INV_WRITE_INTEGRITY), False),
              (f"{form} heartbeat_to", make(A, T, heartbeat_to=0x04), False),
              (f"{form} cancel_backoff", make(A, T, cancel_backoff=0x10), False),
              (f"{form} flag outside the plain set", make(A, T, flags=own | abi.F_PERSIST), False),
              (f"{form} RGB_F_COMPACT already set", make(A, T, flags=own | abi.F_COMPACT), False)]
    # a shape that is none of the three
    t += [("vote reply", record(abi.MSG_REQUEST_VOTE, abi.F_REPLY | abi.F_REPLY_VOTE, (T, 0, 0, 0, A, A)), False),
          ("wrote of another kind", record(abi.MSG_WRITTEN, abi.F_WROTE, (0, A, A, 0, A, A)), False),
          ("failed reply", record(abi.MSG_AER, abi.F_REPLY, (T, A + 1, A, T, A, A)), False)]
    return t


def run_c_decoder(tmp_path, records: bytes) -> bytes:
    """rgb_decision_expand of the header in a stand-alone C program under AddressSanitizer + UBSan."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = tmp_path / "decision_expand_harness"
    cmd = ["gcc", "-std=c11", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
           os.path.join(ROOT, "tests", "native", "decision_expand_harness.c")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert built.returncode == 0, built.stderr
    src, dst = tmp_path / "records.in", tmp_path / "records.out"
    src.write_bytes(records)
    ran = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stderr[-2000:]
    assert int(ran.stdout) == len(records) // 64
    return dst.read_bytes()


def as_slot(compact: bytes) -> bytes:
    """A compact record in its 64-byte slot; the other half holds what the buffer held."""
    return compact + b"\xEE" * 32


def test_codec_known_answers(tmp_path):
    names, stream, want = [], b"", b""
    for base, A, T in BASES:
        for row, full, fits in codec_table(A, T):
            tag = f"{row} ({base})"
            c = compact_ref(full)
            assert (c is not None) == fits, f"{tag}: compact_ref says {'fits' if c else 'does not fit'}"
            if re.fullmatch(r"(confirmed|wrote) \w+=-?\d+|counted fits|\w+ flag outside the plain set", row):
                assert row in rows_of(full), f"{tag}: the record does not land on its own row: {rows_of(full)}"
            if fits:
                assert len(c) == 32 and struct.unpack_from("<I", c, 8)[0] & abi.F_COMPACT
                slot = np.frombuffer(as_slot(c), dtype=abi.DECISION_DTYPE)
                got = abi.expand_decisions(slot)
                assert got.tobytes() == full.tobytes(), f"{tag}: abi.expand_decisions gives\n {got[0]}\n for\n {full}"
                names.append(tag); stream += as_slot(c); want += full.tobytes()
            if not int(full["flags"]) & abi.F_COMPACT:
                # a full record passes through a decoder untouched (fitting ones too: a consumer may expand twice)
                got = abi.expand_decisions(np.frombuffer(full.tobytes(), dtype=abi.DECISION_DTYPE))
                assert got.tobytes() == full.tobytes(), f"{tag}: abi.expand_decisions changed a full record"
                names.append(tag + " in full"); stream += full.tobytes(); want += full.tobytes()
    # the array form decodes a mixed stream record by record
    assert abi.expand_decisions(np.frombuffer(stream, dtype=abi.DECISION_DTYPE)).tobytes() == want
    got = run_c_decoder(tmp_path, stream)
    assert len(got) == len(want)
    for k, tag in enumerate(names):
        g, w = got[64 * k:64 * k + 64], want[64 * k:64 * k + 64]
        assert g == w, (f"{tag}: rgb_decision_expand gives\n {np.frombuffer(g, dtype=abi.DECISION_DTYPE)[0]}\n for\n "
                        f"{np.frombuffer(w, dtype=abi.DECISION_DTYPE)[0]}")


# ------------------------------------------------------------------------------------------ A2: states for the rows

# pattern k of the pattern tick's shard k: which of the 64 lanes of the slice hold a record that fits
SLICE_PATTERNS = [[True] * 64, [False] * 64, [j % 2 == 0 for j in range(64)]] + \
                 [[j != p for j in range(64)] for p in (0, 31, 32, 63)] + [[j == 5 for j in range(64)]]
GAPS = [254, 255, 256, 257, 511, 512, 513, 1022, 1023, 1024, 1025]
BIG_GAPS = [65534, 65535, 65536, 65537]
# (d1, d2, d3, d4) of a written event's reply: every row of the confirmed form, fitting and not
FIT = [(255, 1, 510, 5), (3, 15, 510, 5), (3, 1, 0, 5), (3, 1, 1023, 5), (3, 1, 510, 1023), (3, 1, 510, 0), (254, 14, 1, 1022),
       (0, 0, 512, 1), (255, 15, 1023, 1023), (3, 2, 510, 254), (3, 2, 510, 511), (3, 2, 510, 513), (3, 2, 510, 257)]
NOFIT = [(256, 1, 510, 5), (3, 16, 510, 5), (3, 1, 1024, 5), (3, 1, -1, 5), (3, 1, 510, 1024), (3, 1, 510, -1),
         (3, -1, 510, 5), (257, 1, 510, 5), (3, 17, 510, 5), (3, 1, -2, 5), (3, 1, 1025, 1025)] + \
        [(g, 1, 510, 5) for g in GAPS[2:]] + [(3, 1, 510, g) for g in GAPS[9:]]
BIG = [(g, 1, 510, 5) for g in BIG_GAPS] + [(3, 1, 510, g) for g in BIG_GAPS]     # ranges of 65 k entries: a few servers only

GROUPS = {1: 528, 3: 192, 5: 130, 8: 80}      # 64 followers per shard for the pattern tick, and a ragged tail of groups
REACHABLE = {f"confirmed {k}={v}" for k in ("d1", "d2", "d3", "d4") for v in (0, LIMITS[k], LIMITS[k] + 1, -1)} | \
            {"wrote span=65535", "wrote span=65536", "wrote lag=65535", "wrote lag=65536", "wrote span=0", "wrote lag=0",
             "counted fits", "confirmed flag outside the plain set", "wrote flag outside the plain set",
             "counted flag outside the plain set"}


def pattern_servers(G, N):
    """[shard][lane] -> server: the first 64 servers of every shard (group mod 8) among the groups that hold only
    followers -- the groups below n_pattern_groups."""
    per_shard = -(-64 // N)                     # groups per shard that give 64 servers
    gp = per_shard * 8
    assert gp < G
    out = [[g * N + k for g in range(s, gp, 8) for k in range(N)][:64] for s in range(8)]
    assert all(len(x) == 64 for x in out)
    return out, gp


def build_states(G, N, X, Y):
    """Followers whose next written event answers with the deltas of FIT / NOFIT / BIG, laid out by SLICE_PATTERNS;
    the groups behind them keep a leader in slot 0.  X, Y: where the indexes and the terms of the case lie."""
    st = abi.empty_server_states(G, N)
    lanes, gp = pattern_servers(G, N)
    params = {}
    n_fit = n_no = n_big = 0
    for s in range(8):
        for j in range(64):
            if SLICE_PATTERNS[s][j]:
                params[lanes[s][j]] = FIT[n_fit % len(FIT)]; n_fit += 1
            elif s == 1 and j < 2 * len(BIG):
                params[lanes[s][j]] = BIG[n_big % len(BIG)]; n_big += 1
            else:
                params[lanes[s][j]] = NOFIT[n_no % len(NOFIT)]; n_no += 1
    for srv in range(G * N):
        g, k = divmod(srv, N)
        d1, d2, d3, d4 = params.get(srv, FIT[srv % len(FIT)] if srv % 3 else NOFIT[srv % len(NOFIT)])
        li = X + 70_000 + 13 * srv
        t0 = Y + 20 + srv % 5
        depth = max(d1, d4, 8) + 12                       # the range holds last_written and last_applied
        first = li - depth
        lw_old = li - max(d1, 0) - 6                      # written so far; the event confirms up to li - d1
        st["first_index"][srv], st["last_index"][srv], st["last_term"][srv] = first, li, t0
        st["n_runs"][srv] = 2
        st["run_start"][srv, :2] = (first, first + 3)
        st["run_term"][srv, :2] = (t0 - 1, t0)
        st["last_written_index"][srv], st["last_written_term"][srv] = lw_old, t0
        st["pending_first"][srv] = lw_old + 1
        st["current_term"][srv] = t0 + d2
        st["commit_index"][srv] = li + d3 - 512
        st["last_applied"][srv] = li + 1 - d4
        st["leader_id"][srv] = st["voted_for"][srv] = 0
        for j in range(N):
            st["match_index"][srv, j] = li - 2 - j
            st["next_index"][srv, j] = li - 1
            st["commit_index_sent"][srv, j] = li - 600
        if g >= gp and k > 0 or g >= gp and g % 2 == 1:
            if srv % 2:                                   # last_written_index above last_index: the reply's d1 is -1
                st["last_written_index"][srv], st["pending_first"][srv] = li + 1, li + 1
        if g >= gp and k == 0 and g % 2 == 0:
            st["role"][srv] = abi.ROLE_LEADER
            st["current_term"][srv] = t0                  # a leader commits entries of its own term
            st["commit_index"][srv] = st["last_applied"][srv] = li - 9
    return st, params, lanes, gp


def in_bucket_order(engine, msgs, N):
    b = engine.train_bucket(msgs["kind"], msgs["flags"], msgs["server"], N)
    return msgs[np.argsort(b, kind="stable")]


def msg(server, kind, frm=0, flags=0, term=0, a=0, b=0, c=0, n=0, t_entries=0):
    m = np.zeros(1, dtype=abi.MSG_DTYPE)
    m["server"], m["kind"], m["from"], m["flags"], m["term"], m["a"], m["b"], m["c"] = server, kind, frm, flags, term, a, b, c
    m["n_entries"], m["n_run0"], m["run0_term"], m["run1_term"] = n, n, t_entries, t_entries
    return m[0]


def tick_written(cur, servers, params=None):
    """written events over the pending range of `servers`, up to last_index - d1 for the pattern servers"""
    out = []
    for s in servers:
        row = cur[s]
        li, pf = int(row["last_index"]), int(row["pending_first"])
        to = li - max(params[s][0], 0) if params and s in params else li
        if pf > to:
            continue
        out.append(msg(s, abi.MSG_WRITTEN, term=int(row["last_term"]), a=pf, b=to))
    return out


def tick_appends(cur, followers, leaders, N, big):
    """append_entries_rpc from the leader the follower knows, in its term: leader_commit from last_index - 514 to
    + 513 with 0, 1 or 2 entries (new ones, and ones the log holds); on the `big` servers one new entry with a low
    leader_commit (last_applied stays 65 k behind: the lag of the wrote form) or 65 536 / 65 537 entries (its span); a
    few of a higher term (RGB_F_PERSIST: a flag outside the plain set).  Success replies to the leaders."""
    out = []
    commits = list(range(-514, -509)) + [-2, 0, 1] + list(range(509, 514))
    for q, s in enumerate(followers):
        row = cur[s]
        li, lt, ct, la = int(row["last_index"]), int(row["last_term"]), int(row["current_term"]), int(row["last_applied"])
        if ct < lt or la > li:
            continue                                       # the rows of states no server holds end with the first tick
        term = ct + 1 if q % 23 == 22 else ct
        which = big.index(s) if s in big else -1
        if which >= 0 and which % 8 >= 4:                                 # lag: last_applied 65 k behind, 1 or 2 new entries, nothing applied
            out.append(msg(s, abi.MSG_AER, term=term, a=li, b=lt, c=min(la, li), n=1 + which // 8, t_entries=ct))
            continue
        if which >= 8:                                     # span: 65 536 and 65 537 entries, all applied
            n = 65536 + which % 2
            out.append(msg(s, abi.MSG_AER, term=term, a=li, b=lt, c=li + n, n=n, t_entries=ct))
            continue
        if int(row["last_written_index"]) > li:
            out.append(msg(s, abi.MSG_AER, term=ct, a=li, b=lt, c=li))
            continue
        c = li + commits[q % len(commits)]
        mode = q % 4
        if mode == 0:
            out.append(msg(s, abi.MSG_AER, term=term, a=li, b=lt, c=c))                                   # empty
        elif mode == 1:
            out.append(msg(s, abi.MSG_AER, term=term, a=li - 2, b=lt, c=c, n=2, t_entries=lt))           # both held
        else:
            out.append(msg(s, abi.MSG_AER, term=term, a=li, b=lt, c=c, n=mode - 1, t_entries=ct))        # 1 or 2 new
    for q, s in enumerate(leaders):
        row = cur[s]
        peer = 1 + q % max(N - 1, 1) if N > 1 else 0
        last = int(row["last_written_index"]) - q % 3
        out.append(msg(s, abi.MSG_AER_REPLY, frm=peer, flags=abi.MF_SUCCESS, term=int(row["current_term"]) + (q % 4 == 3), a=last + 1, b=last,
                       c=int(row["last_term"])))
    return out


def build_ticks(engine, O, N, X, Y):
    """The checker's run: (start state, [(msgs, decisions, rpcs, state after)] per tick, the pattern tick's lanes)."""
    G = GROUPS[N]
    st, params, lanes, gp = build_states(G, N, X, Y)
    leaders = [g * N for g in range(gp, G, 2)]
    followers = [s for s in range(G * N) if s not in set(leaders)]
    big = [lanes[1][j] for j in range(2 * len(BIG))]
    cpu = O.Oracle(G, N, max_runs=16)
    cpu.set_state(0, st)
    ticks = []

    def run(msgs):
        msgs = in_bucket_order(engine, np.array(msgs, dtype=abi.MSG_DTYPE), N)
        d, r = cpu.step(msgs)
        ticks.append((msgs, d, r.copy(), cpu.get_state()))

    # 1. the pattern tick: 8 x 64 written events in shard order, then (another class: behind them) the leaders' pipelines
    run(tick_written(st, [s for sh in lanes for s in sh], params) +
        [msg(s, abi.MSG_PIPELINE_RPCS) for s in leaders])
    assert [int(x) for x in ticks[0][0]["server"][:512]] == [s for sh in lanes for s in sh]
    # 2. append_entries_rpc to every follower, success replies to the leaders
    run(tick_appends(ticks[-1][3], followers, leaders, N, big))
    # 3. written events over what is pending now, everywhere
    run(tick_written(ticks[-1][3], range(G * N)))
    # 4. the leaders' followers confirm again; the leaders count
    run(tick_appends(ticks[-1][3], followers[::2], leaders, N, big=[]))
    cpu.close()
    return G, st, ticks, lanes


def coverage(ticks):
    seen = {}
    for _, dec, _, _ in ticks:
        for r in dec:
            for row in rows_of(r):
                seen[row] = seen.get(row, 0) + 1
    return seen


def check_coverage_and_patterns(ticks, tag):
    """From the checker's decisions alone: every reachable row of A1 was produced, and the pattern tick's slices hold
    the patterns."""
    seen = coverage(ticks)
    missing = sorted(REACHABLE - set(seen))
    assert not missing, f"{tag}: rows of the codec table that no decision of the checker landed on: {missing}\n seen: {seen}"
    fits = [compact_ref(r) is not None for r in ticks[0][1][:512]]
    for s in range(8):
        assert fits[64 * s:64 * s + 64] == SLICE_PATTERNS[s], f"{tag}: slice {s} of the pattern tick: {fits[64 * s:64 * s + 64]}"
    shapes = {}
    for _, dec, _, _ in ticks:
        for r in dec:
            f = shape_of(r)
            if f is not None and not (int(r["invariant"]) or int(r["heartbeat_to"]) or int(r["cancel_backoff"])):
                key = (f, compact_ref(r) is not None)
                shapes[key] = shapes.get(key, 0) + 1
    for key in (("confirmed", True), ("confirmed", False), ("wrote", True), ("wrote", False), ("counted", True)):
        assert shapes.get(key, 0) > 0, f"{tag}: no {key[0]}-shaped decision that {'fits' if key[1] else 'does not fit'}: {shapes}"


class Buf:
    """`nbytes` the library can use as DEVICE memory: a CUDA tensor on the GPU, numpy on the emulation."""

    def __init__(self, nbytes, on_gpu, fill=0):
        self.on_gpu = on_gpu
        if on_gpu:
            import torch
            self.t = torch.full((max(nbytes, 16),), fill, dtype=torch.uint8, device="cuda")
            self.ptr = self.t.data_ptr()
        else:
            self.a = np.full(max(nbytes, 16), fill, dtype=np.uint8)
            self.ptr = self.a.ctypes.data

    def put(self, off, data: bytes):
        src = np.frombuffer(data, dtype=np.uint8)
        if self.on_gpu:
            import torch
            self.t[off:off + len(src)] = torch.from_numpy(src.copy()).cuda()
        else:
            self.a[off:off + len(src)] = src

    def host(self):
        return self.t.cpu().numpy() if self.on_gpu else self.a


def assert_state_equal(tag, got, want):
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()]
        diff = [n for n in got.dtype.names if np.any(got[bad[0]][n] != want[bad[0]][n])]
        raise AssertionError(f"{tag}: state of server {bad[0]} differs in {diff} ({len(bad)} servers differ)")


def assert_raw_stream(tag, raw: np.ndarray, msgs, want):
    """One tick's slots of a device-resident decision stream (uint8[n_slots, 64], filled with 0xEE before the launch):
    (a) expanded = the checker's, (b) RGB_F_COMPACT exactly where compact_ref fits, (c) the half a compact record does
    not own still holds 0xEE -- and so does every slot behind the tick."""
    n = len(want)
    rec = raw[:n].reshape(-1).view(abi.DECISION_DTYPE)
    got = abi.expand_decisions(rec)
    for i in range(n):
        c = compact_ref(want[i])
        where = f"{tag}: slot {i} (lane {i % 64}) msg={msgs[i]}"
        is_c = bool(int(rec["flags"][i]) & abi.F_COMPACT)
        assert is_c == (c is not None), f"{where}: RGB_F_COMPACT {'set' if is_c else 'not set'}, compact_ref: {c is not None}\n want={want[i]}"
        if c is not None:
            assert raw[i, :32].tobytes() == c, f"{where}: compact bytes {raw[i, :32].tobytes().hex()} != {c.hex()}"
            assert np.all(raw[i, 32:] == 0xEE), f"{where}: the upper half of a compact record was written: {raw[i, 32:].tobytes().hex()}"
        assert got[i].tobytes() == want[i].tobytes(), f"{where}:\n got ={got[i]}\n want={want[i]}"
    assert np.all(raw[n:] == 0xEE), f"{tag}: a slot behind the tick's {n} records was written"


def rpc_slots(raw_rpcs: np.ndarray, dec, per):
    """The valid records of a tick's fixed rpc slots (message i owns `per` slots, the first n_rpcs count), msg_index
    dropped."""
    slots = raw_rpcs.view(abi.RPC_DTYPE)
    out = [slots[i * per:i * per + int(k)] for i, k in enumerate(dec["n_rpcs"]) if k]
    r = np.concatenate(out + [np.zeros(0, dtype=abi.RPC_DTYPE)]).copy()
    r["msg_index"] = 0
    return r


def check_decision_paths(engine, O, N, X, Y, on_gpu):
    import fuzz
    tag0 = f"N={N} indexes from {X:#x} terms from {Y:#x}"
    G, st0, ticks, lanes = build_ticks(engine, O, N, X, Y)
    check_coverage_and_patterns(ticks, tag0)            # before anything touches an engine
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

    with engine.RaGpuBatch(G, N, max_runs=16, ring_slots=2, ring_capacity=max(1024, S)) as eng:
        # 1, 2: rgb_run_ticks_device, kind-generic and class kernels, tick by tick (the rpc slots are per tick)
        for name, kc in (("generic kernel", None), ("class kernels", kinds)):
            eng.set_state(0, st0)
            for t in range(T):
                ddec, drpc = Buf(tb, on_gpu, 0xEE), Buf(rs, on_gpu)
                eng.run_ticks_device(dmsgs.ptr + t * tb, S, 1, ddec.ptr, drpc.ptr, tick_counts=counts[t:t + 1],
                                     kind_counts=None if kc is None else kc[t:t + 1])
                eng.synchronize()
                tag = f"{tag0}, {name}, tick {t}"
                assert_raw_stream(tag, ddec.host()[:tb].reshape(S, 64), ticks[t][0], ticks[t][1])
                assert rpc_slots(drpc.host()[:rs], ticks[t][1], per).tobytes() == want_rpcs(t).tobytes(), tag + ": rpc records"
                assert_state_equal(tag, eng.get_state(), ticks[t][3])
        # 3: one train launch over all ticks
        eng.set_state(0, st0)
        plan = eng.train_plan(buckets)
        stamps, ddec, drpc = Buf(T * S, on_gpu), Buf(T * tb, on_gpu, 0xEE), Buf(T * rs, on_gpu)
        eng.train_stamp_device(dmsgs.ptr, stamps.ptr, S, counts)
        eng.train_run_device(plan, 0, T, dmsgs.ptr, stamps.ptr, S, ddec.ptr, drpc.ptr, rpc_ring=T)
        eng.synchronize()
        assert eng.train_status()[0] == 0
        for t in range(T):
            tag = f"{tag0}, train, tick {t}"
            assert_raw_stream(tag, ddec.host()[t * tb:(t + 1) * tb].reshape(S, 64), ticks[t][0], ticks[t][1])
            assert rpc_slots(drpc.host()[t * rs:(t + 1) * rs], ticks[t][1], per).tobytes() == want_rpcs(t).tobytes(), tag + ": rpc records"
        assert_state_equal(f"{tag0}, train", eng.get_state(), ticks[-1][3])
        plan.close()
        # 4, 5: the host paths -- rgb_results_kernel expands on the device
        for name, step in (("rgb_submit", eng.step), ("rgb_submit_raw", lambda m: eng.step_raw(m, max_rounds=1))):
            eng.set_state(0, st0)
            for t in range(T):
                tag = f"{tag0}, {name}, tick {t}"
                dg, rg = step(ticks[t][0])
                for i in np.flatnonzero((dg.view(np.uint8).reshape(-1, 64) != ticks[t][1].view(np.uint8).reshape(-1, 64)).any(axis=1))[:1]:
                    raise AssertionError(f"{tag}: record {i} msg={ticks[t][0][i]}\n got ={dg[i]}\n want={ticks[t][1][i]}")
                assert len(dg) == len(ticks[t][1])
                assert fuzz.sort_rpcs(rg.copy()).tobytes() == fuzz.sort_rpcs(ticks[t][2]).tobytes(), tag + ": rpc records"
                assert_state_equal(tag, eng.get_state(), ticks[t][3])


# N in {1, 3, 5, 8}; small values, indexes that cross 2^32 inside the case, indexes and terms above 2^63
CASES = [(5, 0, 0), (1, 0, 0), (3, 2**32 - 70_300, 2**32 - 22), (8, 2**63 - 1000, 2**63 - 21)]


@pytest.mark.parametrize("n_members,index_base,term_base", CASES)
def test_decision_paths_on_the_block_emulation(emulated_engine, oracle_lib, n_members, index_base, term_base):
    check_decision_paths(emulated_engine, oracle_lib, n_members, index_base, term_base, False)


@pytest.mark.gpu
@pytest.mark.parametrize("n_members,index_base,term_base", CASES)
def test_gpu_decision_paths(gpu_engine, oracle_lib, n_members, index_base, term_base):
    check_decision_paths(gpu_engine, oracle_lib, n_members, index_base, term_base, True)
