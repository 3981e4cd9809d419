"""The compact decision forms of RGB_ABI_MINOR 1 (include/ra_gpu_batch.h, "Compact decisions"): counted for more kinds
and with a query index, wrote and confirmed with the flags of a change, answered, stood.

B1 pins the codec.  compact_ref() is the encoder written from the header's comment alone, in Python's integers (it
restates the three forms tests/test_compact_decisions.py pins and adds the new ones); a table of full records holds, per
new form, both sides of every threshold (a difference at its limit and at limit + 1), a negative difference, zero
differences, UINT64_MAX in each of the six words and a zero anchor; abi.compact_forms must classify every record as
compact_ref does, abi.expand_decisions must give every compacted record back, and rgb_decision_expand (a stand-alone C
program under AddressSanitizer + UBSan, tests/native/compact_forms_harness.c) must agree with abi.expand_decisions.

B2 pins the device's encoder and decoders.  States and messages are built so that the CHECKER's decisions land on the
rows of B1 (asserted from the checker's decisions alone, before an engine is touched); the same ticks then run through
rgb_run_ticks_device (kind-generic and class kernels), both train forms (a host-built plan: dealt; a device-built plan:
persistent), rgb_submit and rgb_submit_raw.  Raw streams must hold RGB_F_COMPACT exactly where compact_ref fits, the 32
bytes compact_ref gives, an untouched upper half, and expand to the checker's records bit for bit.  8 groups x 5 (every
scenario once, over several one-tick rounds) and 260 groups x 5 (one tick, every scenario many times: the slices of 64
mix new-form, old-form and full records, which is asserted).

B3: 32 ticks of the closed loop (the load generator on the engine, 64 x 5): every tick's expanded decisions and the
final state equal the checker's.

Every check is a plain function of an engine module: once on the emulated library, once (`-m gpu`) on the device."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from ra_amd import abi
from test_compact_decisions import Buf, assert_state_equal, in_bucket_order, msg, rpc_slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2**64 - 1


@pytest.fixture(scope="module")
def gpu_engine():
    from ra_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build()    # a fresh checkout on the GPU box: hipcc is there, the .so is not in git
    engine.lib()          # raises if the HIP library is missing: no fallback
    return engine


# ------------------------------------------------------------------------------------------ the encoder, from the header

PLAIN = abi.F_LEADER_MSG | abi.F_APPLIED | abi.F_AUX_EVAL | abi.F_PIPELINE
CHANGE = abi.F_PERSIST | abi.F_LEADER_CHANGED | abi.F_REPROCESSED | abi.F_ROLE_CHANGED
CONFIRMED = abi.F_REPLY | abi.F_REPLY_SUCCESS
BECAME = abi.F_BECAME_LEADER | abi.F_ROLE_CHANGED | abi.F_LEADER_CHANGED
COUNTED_KINDS = (abi.MSG_AER_REPLY, abi.MSG_WRITTEN, abi.MSG_AER, abi.MSG_VOTE_RESULT, abi.MSG_APPEND,
                 abi.MSG_PRE_VOTE_RESULT, abi.MSG_SNAPSHOT_WRITTEN, abi.MSG_HEARTBEAT_RPC)
WORDS = ("reply_term", "reply_next_index", "reply_last_index", "reply_last_term", "commit_index", "last_applied")
# form -> the differences it stores and their limits (each lies in 0..limit, in the integers)
LIMITS = {"counted": {}, "counted q": {"q": 2**32 - 1}, "wrote": {"span": 0xFFFF, "lag": 0xFFFF},
          "confirmed": {"d1": 0xFF, "d2": 0xF, "d3": 0x3FF, "d4": 0x3FF}, "answered": {"q": 0xFFFF, "dl": 0xFFFF},
          "stood": {"dt": 0xFF, "dc": 0xFFF, "da": 0xFFF}}
NEW_FORMS = ("counted q", "answered", "stood")


def form_of(r):
    """The form kind and flags name, or None."""
    kind, shape = int(r["kind"]), int(r["flags"]) & ~PLAIN & ~abi.F_COMPACT
    stem = shape & ~CHANGE
    aer = kind == abi.MSG_AER and (stem == shape or shape & (abi.F_ROLE_CHANGED | abi.F_LEADER_CHANGED))
    if (shape == 0 and kind in COUNTED_KINDS) or (kind == abi.MSG_VOTE_RESULT and shape == BECAME):
        return "counted"
    if kind == abi.MSG_HEARTBEAT_REPLY and shape == abi.F_QUERY_QUORUM:
        return "counted q"
    if stem == abi.F_WROTE and aer:
        return "wrote"
    if stem == CONFIRMED and (aer or (kind == abi.MSG_WRITTEN and stem == shape)):
        return "confirmed"
    if kind == abi.MSG_HEARTBEAT_RPC and stem == abi.F_REPLY | abi.F_REPLY_HEARTBEAT:
        return "answered"
    if kind == abi.MSG_PRE_VOTE_RESULT and stem == abi.F_SEND_VOTE_REQUESTS:
        return "stood"
    return None


def deltas(form, r):
    term, nxt, last, lterm, ci, la = (int(r[f]) for f in WORDS)
    if form == "counted q":
        return {"q": nxt}
    if form == "wrote":
        return {"span": last - nxt, "lag": last - la}
    if form == "confirmed":
        return {"d1": nxt - 1 - last, "d2": term - lterm, "d3": ci + 512 - (nxt - 1), "d4": nxt - la}
    if form == "answered":
        return {"q": nxt, "dl": ci + 32768 - la}
    if form == "stood":
        return {"dt": term - lterm, "dc": last - ci, "da": last - la}
    return {}


def zero_words(form, r):
    """The words the form does not store are 0 (and reply_next_index is not, where A = reply_next_index - 1)."""
    term, nxt, last, lterm, ci, la = (int(r[f]) for f in WORDS)
    return {"counted": not (term or nxt or last or lterm), "counted q": not (term or last or lterm),
            "wrote": not (term or lterm), "confirmed": nxt != 0, "answered": not (last or lterm), "stood": nxt == 0}[form]


def compact_ref(r):
    """The 32 bytes the header describes for the full record r (one abi.DECISION_DTYPE record), or None when r is
    written in full."""
    flags = int(r["flags"])
    if int(r["invariant"]) or int(r["heartbeat_to"]) or int(r["cancel_backoff"]) or flags & abi.F_COMPACT:
        return None
    form = form_of(r)
    if form is None or not zero_words(form, r):
        return None
    d = deltas(form, r)
    if any(not 0 <= d[k] <= lim for k, lim in LIMITS[form].items()):
        return None
    term, nxt, last, lterm, ci, la = (int(r[f]) for f in WORDS)
    aux, A, B = {"counted": lambda: (0, ci, la), "counted q": lambda: (d["q"], ci, la),
                 "wrote": lambda: (d["span"] | d["lag"] << 16, last, ci),
                 "confirmed": lambda: (d["d1"] | d["d2"] << 8 | d["d3"] << 12 | d["d4"] << 22, nxt - 1, term),
                 "answered": lambda: (d["q"] | d["dl"] << 16, ci, term),
                 "stood": lambda: (d["dt"] | d["dc"] << 8 | d["da"] << 20, last, term)}[form]()
    return r.tobytes()[:8] + struct.pack("<IIQQ", flags | abi.F_COMPACT, aux, A, B)


def rows_of(r):
    """The rows of the B1 table a full record lands on.  A threshold row ('answered dl=65536') counts only when every
    other difference of the form fits: the named one alone decides."""
    out = set()
    if int(r["invariant"]) or int(r["heartbeat_to"]) or int(r["cancel_backoff"]):
        return out
    form, kind, shape = form_of(r), int(r["kind"]), int(r["flags"]) & ~PLAIN
    if form is None:
        if kind == abi.MSG_AER and shape == abi.F_WROTE | abi.F_PERSIST:
            out.add("wrote with RGB_F_PERSIST alone stays full")
        if kind == abi.MSG_REQUEST_VOTE and shape & ~CHANGE & ~abi.F_REPLY_SUCCESS == abi.F_REPLY | abi.F_REPLY_VOTE:
            out.add("a vote reply stays full, " + ("granted" if shape & abi.F_REPLY_SUCCESS else "denied"))
        return out
    if not zero_words(form, r):
        return out
    d = deltas(form, r)
    for k, lim in LIMITS[form].items():
        if all(0 <= d[o] <= LIMITS[form][o] for o in LIMITS[form] if o != k):
            for v in (0, lim, lim + 1, -1):
                if d[k] == v:
                    out.add(f"{form} {k}={v}")
    if compact_ref(r) is not None:
        if form == "counted":
            out.add(f"counted kind {kind}" + (" became leader" if shape else ""))
        if form in ("wrote", "confirmed", "answered", "stood") and shape & CHANGE:
            out.add(f"{form} with the flags of a change")
        if form == "answered":
            out.add("answered heartbeat")
    return out


def record(kind, flags, words, server=7, role=abi.ROLE_FOLLOWER, reply_to=2, **kw):
    r = np.zeros(1, dtype=abi.DECISION_DTYPE)
    r["server"], r["role"], r["reply_to"], r["kind"], r["flags"] = server, role, reply_to, kind, flags
    for f, v in zip(WORDS, words):
        r[f] = v % 2**64
    for f, v in kw.items():
        r[f] = v
    return r[0]


def answered(A, T, q=3, dl=32768 + 7, kind=abi.MSG_HEARTBEAT_RPC, flags=abi.F_REPLY | abi.F_REPLY_HEARTBEAT, **kw):
    return record(kind, flags, (T, q, 0, 0, A, A + 32768 - dl), **kw)


def stood(A, T, dt=2, dc=80, da=90, flags=abi.F_SEND_VOTE_REQUESTS | abi.F_ROLE_CHANGED | abi.F_PERSIST, **kw):
    return record(abi.MSG_PRE_VOTE_RESULT, flags, (T, 0, A, T - dt, A - dc, A - da), role=abi.ROLE_CANDIDATE, reply_to=abi.NONE, **kw)


def counted_q(A, T, q=5, **kw):
    return record(abi.MSG_HEARTBEAT_REPLY, abi.F_QUERY_QUORUM, (0, q, 0, 0, A, A - 3), role=abi.ROLE_LEADER, reply_to=abi.NONE, **kw)


def counted(A, T, kind, flags=0, **kw):
    return record(kind, flags, (0, 0, 0, 0, A, A - 3), reply_to=abi.NONE, **kw)


BASES = [("small", 70_000, 300), ("around 2^32", 2**32 + 100, 2**32 + 3), ("around 2^63", 2**63 + 100, 2**63 + 3)]
MAKERS = {"answered": answered, "stood": stood, "counted q": counted_q}
UMAX_FITS = {("answered", "reply_term"), ("counted q", "commit_index"), ("counted q", "last_applied")}


def codec_table(A, T):
    """(row, full record, fits) -- per new form both sides of every threshold, negative and zero differences,
    UINT64_MAX in each word, a zero anchor; the extended kinds and flag sets of the forms that were there."""
    t = []
    for form in NEW_FORMS:
        make = MAKERS[form]
        for k, lim in LIMITS[form].items():
            t += [(f"{form} {k}={lim}", make(A, T, **{k: lim}), True), (f"{form} {k}={lim + 1}", make(A, T, **{k: lim + 1}), False),
                  (f"{form} {k}=0", make(A, T, **{k: 0}), True)]
            if k != "q":
                t.append((f"{form} {k}=-1", make(A, T, **{k: -1}), False))
        t.append((f"{form} every field at its limit", make(A, T, **LIMITS[form]), True))
        # UINT64_MAX in each word of a record that fits otherwise.  It fits only as an anchor nothing is measured from
        # (answered's B = reply_term, counted q's A and B); as a stored word it is non-zero or beyond its field, as an
        # anchor with differences it leaves them negative or beyond their fields
        base = make(A, T)
        for w in WORDS:
            r = base.copy()
            r[w] = U64
            t.append((f"{form} {w} = UINT64_MAX", r, (form, w) in UMAX_FITS))
        t += [(f"{form} invariant", make(A, T, invariant=abi.INV_WRITE_INTEGRITY), False),
              (f"{form} heartbeat_to", make(A, T, heartbeat_to=0x04), False),
              (f"{form} cancel_backoff", make(A, T, cancel_backoff=0x10), False)]
    # zero anchors, and UINT64_MAX in both anchors with the differences on the far side of the wrap
    t += [("answered A = 0", answered(0, T, dl=32768), True), ("answered A = 0, applied above", answered(0, T, dl=0), True),
          ("answered A = 0, B = 0", answered(0, 0, dl=32768), True), ("answered A = 32767, dl at its limit", answered(32767, T, dl=0xFFFF), True),
          ("answered A = 32766 cannot hold dl = 65535", answered(32766, T, dl=0xFFFE), True),
          ("answered anchors = UINT64_MAX", answered(U64, U64, dl=32768 + 5), True),
          ("answered applied wraps past UINT64_MAX", record(abi.MSG_HEARTBEAT_RPC, abi.F_REPLY | abi.F_REPLY_HEARTBEAT, (T, 1, 0, 0, U64, 4)), False),
          ("stood A = 0", stood(0, T, dc=0, da=0), True), ("stood B = 0", stood(A, 0, dt=0), True),
          ("stood anchors = UINT64_MAX", stood(U64, U64), True), ("stood next is not 0", record(abi.MSG_PRE_VOTE_RESULT, abi.F_SEND_VOTE_REQUESTS, (T, 1, A, T, A, A)), False),
          ("counted q A = 0, B = 0", record(abi.MSG_HEARTBEAT_REPLY, abi.F_QUERY_QUORUM, (0, 9, 0, 0, 0, 0)), True),
          ("counted q anchors = UINT64_MAX", record(abi.MSG_HEARTBEAT_REPLY, abi.F_QUERY_QUORUM, (0, 9, 0, 0, U64, U64)), True),
          ("counted q with a term", record(abi.MSG_HEARTBEAT_REPLY, abi.F_QUERY_QUORUM, (T, 9, 0, 0, A, A)), False),
          ("answered with a last index", record(abi.MSG_HEARTBEAT_RPC, abi.F_REPLY | abi.F_REPLY_HEARTBEAT, (T, 1, A, 0, A, A)), False)]
    # vote replies stay full (tests/test_compact_decisions.py holds one as a shape that is none of the forms)
    for name, f in (("vote granted", abi.F_REPLY | abi.F_REPLY_VOTE | abi.F_REPLY_SUCCESS | abi.F_PERSIST),
                    ("vote denied", abi.F_REPLY | abi.F_REPLY_VOTE), ("vote granted, stepped down", abi.F_REPLY | abi.F_REPLY_VOTE | abi.F_REPLY_SUCCESS | CHANGE)):
        t.append((f"a vote reply, {name}", answered(A, T, q=0, kind=abi.MSG_REQUEST_VOTE, flags=f), False))
    t += [("a vote reply of another kind", answered(A, T, q=0, kind=abi.MSG_PRE_VOTE_RPC, flags=abi.F_REPLY | abi.F_REPLY_VOTE), False),
          ("a pre-vote reply", answered(A, T, kind=abi.MSG_PRE_VOTE_RPC, flags=abi.F_REPLY | abi.F_REPLY_PRE_VOTE), False),
          ("answered heartbeat with RGB_F_PERSIST", answered(A, T, flags=abi.F_REPLY | abi.F_REPLY_HEARTBEAT | abi.F_PERSIST | abi.F_LEADER_MSG), True),
          ("stood without the flags of a change", stood(A, T, flags=abi.F_SEND_VOTE_REQUESTS), True),
          ("pre-vote requests", stood(A, T, flags=abi.F_SEND_VOTE_REQUESTS | abi.F_PRE_VOTE_REQS), False)]
    # counted: the kinds of minor 1, every plain flag; the kinds it does not take
    for kind in COUNTED_KINDS:
        t.append((f"counted kind {kind}", counted(A, T, kind, flags=PLAIN), True))
    t += [("counted became leader", counted(A, T, abi.MSG_VOTE_RESULT, flags=BECAME, role=abi.ROLE_LEADER), True),
          ("became leader of another kind", counted(A, T, abi.MSG_PRE_VOTE_RESULT, flags=BECAME), False),
          ("counted pipeline_rpcs", counted(A, T, abi.MSG_PIPELINE_RPCS), False),
          ("counted heartbeat_reply without a quorum", counted(A, T, abi.MSG_HEARTBEAT_REPLY), False),
          ("counted step-down", counted(A, T, abi.MSG_AER_REPLY, flags=abi.F_ROLE_CHANGED | abi.F_LEADER_CHANGED | abi.F_PERSIST), False),
          ("counted append with a word", record(abi.MSG_APPEND, 0, (0, 0, 1, 0, A, A)), False)]
    # wrote and confirmed of an append_entries_rpc: the flags of a change only with a new role or leader among them
    wr = (0, A - 2, A, 0, A - 4, A - 9)
    cf = (T, A + 1, A - 3, T - 1, A - 2, A - 4)
    for name, words, own in (("wrote", wr, abi.F_WROTE), ("confirmed", cf, CONFIRMED)):
        for extra, fits in ((abi.F_REPROCESSED | abi.F_ROLE_CHANGED, True), (abi.F_PERSIST | abi.F_LEADER_CHANGED, True), (CHANGE, True),
                            (abi.F_LEADER_CHANGED, True), (abi.F_PERSIST, False), (abi.F_REPROCESSED, False),
                            (abi.F_PERSIST | abi.F_REPROCESSED, False), (abi.F_ROLE_CHANGED | abi.F_TRUNCATED, False)):
            t.append((f"{name} with flags {extra:#x}", record(abi.MSG_AER, own | extra | abi.F_LEADER_MSG, words), fits))
    t += [("confirmed written with a changed role", record(abi.MSG_WRITTEN, CONFIRMED | abi.F_ROLE_CHANGED, cf), False),
          ("a failed reply", record(abi.MSG_AER, abi.F_REPLY | abi.F_ROLE_CHANGED | abi.F_LEADER_MSG, cf, role=abi.ROLE_AWAIT_CONDITION), False)]
    return t


def as_slot(compact: bytes) -> bytes:
    """A compact record in its 64-byte slot; the other half holds what the buffer held."""
    return compact + b"\xEE" * 32


def run_c_harness(tmp_path, slots: bytes, want: bytes):
    """Every record through rgb_decision_expand, compared in C with what abi.expand_decisions gave.  Built under
    AddressSanitizer + UBSan where their runtime links; without them when it does not -- the comparison is made
    either way, and a missing C compiler is a failure (the checker and the emulation need one too)."""
    assert shutil.which("gcc") is not None, "no gcc: rgb_decision_expand cannot be compared with abi.expand_decisions"
    exe = tmp_path / "compact_forms_harness"
    base = ["gcc", "-std=c11", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
            os.path.join(ROOT, "tests", "native", "compact_forms_harness.c")]
    built = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if built.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, "with sanitizers:\n" + built.stderr[-1500:] + "\nwithout:\n" + plain.stderr[-1500:]
    a, b = tmp_path / "slots.in", tmp_path / "records.want"
    a.write_bytes(slots); b.write_bytes(want)
    ran = subprocess.run([str(exe), str(a), str(b)], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stderr[-2000:]
    assert int(ran.stdout) == len(slots) // 64


def test_abi_minor():
    text = " ".join(open(os.path.join(ROOT, "include", "ra_gpu_batch.h")).read().split())
    assert f"#define RGB_ABI_MINOR {abi.ABI_MINOR}u" in text and abi.ABI_MINOR == 1


def test_codec_known_answers(tmp_path):
    names, stream, want = [], b"", b""
    for base, A, T in BASES:
        for row, full, fits in codec_table(A, T):
            tag = f"{row} ({base})"
            c = compact_ref(full)
            assert (c is not None) == fits, f"{tag}: compact_ref says {'fits' if c else 'does not fit'}: {full}"
            form = int(abi.compact_forms(np.array([full]))[0])
            assert (form != 0) == fits, f"{tag}: abi.compact_forms says {abi.COMPACT_FORM_NAMES[form]}"
            if fits:
                assert abi.COMPACT_FORM_NAMES[form] == form_of(full).split()[0], tag
                assert len(c) == 32 and struct.unpack_from("<I", c, 8)[0] & abi.F_COMPACT
                got = abi.expand_decisions(np.frombuffer(as_slot(c), dtype=abi.DECISION_DTYPE))
                assert got.tobytes() == full.tobytes(), f"{tag}: abi.expand_decisions gives\n {got[0]}\n for\n {full}"
                names.append(tag); stream += as_slot(c); want += full.tobytes()
            got = abi.expand_decisions(np.frombuffer(full.tobytes(), dtype=abi.DECISION_DTYPE))
            assert got.tobytes() == full.tobytes(), f"{tag}: abi.expand_decisions changed a full record"
            names.append(tag + " in full"); stream += full.tobytes(); want += full.tobytes()
    # the table holds, per new form: both sides of every threshold, a negative difference, a zero anchor
    have = {row for row, _, _ in codec_table(70_000, 300)}
    for form in NEW_FORMS:
        for k, lim in LIMITS[form].items():
            assert {f"{form} {k}={lim}", f"{form} {k}={lim + 1}", f"{form} {k}=0"} <= have, (form, k)
            assert k == "q" or f"{form} {k}=-1" in have, (form, k)
        assert {f"{form} {w} = UINT64_MAX" for w in WORDS} <= have and any(r.startswith(form + " A = 0") for r in have), form
    assert abi.expand_decisions(np.frombuffer(stream, dtype=abi.DECISION_DTYPE)).tobytes() == want
    run_c_harness(tmp_path, stream, want)


# ------------------------------------------------------------------------------------------ B2: states for the rows

# what the checker's decisions must land on before an engine is touched
REACHABLE = {f"answered dl={v}" for v in (0, 0xFFFF, 0x10000, -1)} | {"answered q=65535", "answered q=65536"} | \
            {f"stood {k}={v}" for k, lim in LIMITS["stood"].items() for v in (0, lim, lim + 1, -1)} | \
            {"counted q q=4294967295", "counted q q=4294967296", "a vote reply stays full, granted", "a vote reply stays full, denied", "answered heartbeat",
             "answered with the flags of a change", "stood with the flags of a change", "wrote with the flags of a change",
             "confirmed with the flags of a change", "wrote with RGB_F_PERSIST alone stays full"} | \
            {f"counted kind {k}" for k in (abi.MSG_AER_REPLY, abi.MSG_WRITTEN, abi.MSG_VOTE_RESULT, abi.MSG_APPEND,
                                           abi.MSG_PRE_VOTE_RESULT, abi.MSG_SNAPSHOT_WRITTEN)} | \
            {f"counted kind {abi.MSG_VOTE_RESULT} became leader"}
TOKEN = 0x0000_7E57_0000_0077


def follower(st, srv, N, X, Y, depth=4200):
    """A follower of the leader in slot 0 with a written log of `depth` entries; -> (last index, last term, term)."""
    li, t0 = X + 70_000 + 13 * srv, Y + 20 + srv % 5
    first = li - depth
    st["first_index"][srv], st["last_index"][srv], st["last_term"][srv] = first, li, t0
    st["n_runs"][srv] = 2
    st["run_start"][srv, :2] = (first, first + 3)
    st["run_term"][srv, :2] = (t0 - 1, t0)
    st["last_written_index"][srv], st["last_written_term"][srv] = li, t0
    st["pending_first"][srv] = li + 1
    st["current_term"][srv] = t0 + 1
    st["commit_index"][srv], st["last_applied"][srv] = li - 5, li - 9
    st["leader_id"][srv] = st["voted_for"][srv] = 0
    st["pre_vote_token"][srv] = TOKEN
    for j in range(N):
        st["match_index"][srv, j], st["next_index"][srv, j], st["commit_index_sent"][srv, j] = li - 2, li + 1, li - 5
    return li, t0, t0 + 1


def scenarios(N):
    """[(name, f(st, srv, X, Y) -> message)]: each sets up one server and returns the message it gets."""
    quorum = N // 2 + 1
    out = []

    def add(name):
        def deco(f):
            out.append((name, f))
        return deco

    def self_of(srv):
        return srv % N

    def peer(srv, k=1):
        return (self_of(srv) + k) % N

    def set_ci_la(st, srv, ci, la):
        st["commit_index"][srv], st["last_applied"][srv] = ci % 2**64, la % 2**64

    # answered, heartbeat_rpc: last_applied against commit_index on both sides of both ends, the query index at its limit
    for dl in (0, 1, 0xFFFF, 0x10000, -1, 32768):
        @add(f"heartbeat dl={dl}")
        def _(st, srv, X, Y, dl=dl):
            li, lt, ct = follower(st, srv, N, X, Y)
            ci = li - 100
            set_ci_la(st, srv, ci, ci + 32768 - dl)
            return msg(srv, abi.MSG_HEARTBEAT_RPC, frm=0, term=ct, a=4)
    for q in (0xFFFF, 0x10000):
        @add(f"heartbeat q={q}")
        def _(st, srv, X, Y, q=q):
            li, lt, ct = follower(st, srv, N, X, Y)
            st["query_index"][srv] = q - 1
            return msg(srv, abi.MSG_HEARTBEAT_RPC, frm=0, term=ct, a=q)

    @add("heartbeat of a new term and leader")
    def _(st, srv, X, Y):
        li, lt, ct = follower(st, srv, N, X, Y)
        return msg(srv, abi.MSG_HEARTBEAT_RPC, frm=peer(srv, 2) or 1, term=ct + 1, a=2)

    # answered, request_vote_rpc: granted (a higher term, an up-to-date log), denied (voted for another in this term)
    for dl in (0, 0xFFFF, 0x10000, -1, 32768):
        @add(f"vote granted dl={dl}")
        def _(st, srv, X, Y, dl=dl):
            li, lt, ct = follower(st, srv, N, X, Y)
            ci = li - 100
            set_ci_la(st, srv, ci, ci + 32768 - dl)
            return msg(srv, abi.MSG_REQUEST_VOTE, frm=peer(srv), term=ct + 1, a=li, b=lt)

    @add("vote denied")
    def _(st, srv, X, Y):
        li, lt, ct = follower(st, srv, N, X, Y)
        st["voted_for"][srv] = peer(srv, 2) if N > 2 else self_of(srv)
        return msg(srv, abi.MSG_REQUEST_VOTE, frm=peer(srv), term=ct, a=li, b=lt)

    # stood: the pre-vote that completes the quorum; each difference on both sides of both ends
    for k, lim in LIMITS["stood"].items():
        for v in (0, lim, lim + 1, -1):
            @add(f"stood {k}={v}")
            def _(st, srv, X, Y, k=k, v=v):
                li, lt, ct = follower(st, srv, N, X, Y)
                st["role"][srv], st["votes"][srv] = abi.ROLE_PRE_VOTE, quorum - 1
                st["leader_id"][srv] = abi.NONE
                d = {"dt": 2, "dc": 80, "da": 90}
                d[k] = v
                ct = lt + d["dt"] - 1                               # the candidate's term will be ct + 1
                st["current_term"][srv] = ct
                set_ci_la(st, srv, li - d["dc"], li - d["da"])
                return msg(srv, abi.MSG_PRE_VOTE_RESULT, frm=peer(srv), flags=abi.MF_SUCCESS, term=ct, c=TOKEN)

    @add("pre-vote short of the quorum")
    def _(st, srv, X, Y):
        li, lt, ct = follower(st, srv, N, X, Y)
        st["role"][srv], st["votes"][srv], st["leader_id"][srv] = abi.ROLE_PRE_VOTE, max(quorum - 2, 0), abi.NONE
        return msg(srv, abi.MSG_PRE_VOTE_RESULT, frm=peer(srv), flags=0 if quorum < 2 else abi.MF_SUCCESS, term=ct, c=TOKEN)

    # counted: vote results short of and at the quorum, {commands}, snapshot_written, a leader's heartbeat quorum
    for at_quorum in (False, True):
        @add("vote result " + ("at the quorum" if at_quorum else "short of it"))
        def _(st, srv, X, Y, at_quorum=at_quorum):
            li, lt, ct = follower(st, srv, N, X, Y)
            st["role"][srv], st["leader_id"][srv], st["voted_for"][srv] = abi.ROLE_CANDIDATE, abi.NONE, self_of(srv)
            st["votes"][srv] = quorum - 1 if at_quorum else max(quorum - 2, 0)
            return msg(srv, abi.MSG_VOTE_RESULT, frm=peer(srv), flags=abi.MF_SUCCESS if at_quorum or quorum >= 2 else 0, term=ct)

    def leader(st, srv, X, Y):
        li, lt, ct = follower(st, srv, N, X, Y)
        st["role"][srv], st["leader_id"][srv], st["voted_for"][srv] = abi.ROLE_LEADER, self_of(srv), self_of(srv)
        st["current_term"][srv] = lt
        return li, lt, lt

    for n in (1, 3):
        @add(f"commands n={n}")
        def _(st, srv, X, Y, n=n):
            leader(st, srv, X, Y)
            return msg(srv, abi.MSG_APPEND, n=n)

    @add("snapshot written")
    def _(st, srv, X, Y):
        li, lt, ct = follower(st, srv, N, X, Y)
        return msg(srv, abi.MSG_SNAPSHOT_WRITTEN, a=li - 9, b=lt)

    for q in (5, 2**32 - 1, 2**32):
        @add(f"heartbeat quorum q={q}")
        def _(st, srv, X, Y, q=q):
            li, lt, ct = leader(st, srv, X, Y)
            st["query_index"][srv] = q
            st["peer_query_index"][srv, :N] = q
            st["peer_query_index"][srv, peer(srv)] = q - 1
            return msg(srv, abi.MSG_HEARTBEAT_REPLY, frm=peer(srv), term=ct, a=q)

    @add("success reply counted")
    def _(st, srv, X, Y):
        li, lt, ct = leader(st, srv, X, Y)
        return msg(srv, abi.MSG_AER_REPLY, frm=peer(srv), flags=abi.MF_SUCCESS, term=ct, a=li + 1, b=li, c=lt)

    @add("written at a leader, counted")
    def _(st, srv, X, Y):
        li, lt, ct = leader(st, srv, X, Y)
        st["last_written_index"][srv], st["pending_first"][srv] = li - 3, li - 2
        return msg(srv, abi.MSG_WRITTEN, term=lt, a=li - 2, b=li)

    # append_entries_rpc: the forms that were there, and with a new leader / a new term and leader / a new term alone
    for name, frm_k, dterm in (("the leader", 0, 0), ("another leader", 1, 0), ("a new term and leader", 1, 1), ("a new term alone", 0, 1)):
        for n in (0, 2):
            @add(f"append_entries_rpc n={n} from {name}")
            def _(st, srv, X, Y, frm_k=frm_k, dterm=dterm, n=n):
                li, lt, ct = follower(st, srv, N, X, Y)
                if self_of(srv) == 0:                               # the known leader sits in slot 1 for the server of slot 0
                    st["leader_id"][srv] = st["voted_for"][srv] = 1
                frm = (int(st["leader_id"][srv]) + frm_k * 2) % N if N > 2 else int(st["leader_id"][srv])
                if frm == self_of(srv):
                    frm = (frm + 1) % N
                return msg(srv, abi.MSG_AER, frm=frm, term=ct + dterm, a=li, b=lt, c=li, n=n, t_entries=ct + dterm)

    @add("append_entries_rpc of an old term")
    def _(st, srv, X, Y):
        li, lt, ct = follower(st, srv, N, X, Y)
        return msg(srv, abi.MSG_AER, frm=0 if self_of(srv) else 1, term=ct - 1, a=li, b=lt, c=li)

    @add("written, confirmed")
    def _(st, srv, X, Y):
        li, lt, ct = follower(st, srv, N, X, Y)
        st["last_written_index"][srv], st["pending_first"][srv] = li - 3, li - 2
        return msg(srv, abi.MSG_WRITTEN, term=lt, a=li - 2, b=li)

    # full records of other shapes
    @add("election timeout")
    def _(st, srv, X, Y):
        follower(st, srv, N, X, Y)
        return msg(srv, abi.MSG_ELECTION_TIMEOUT, c=TOKEN + 1)

    @add("consistent query")
    def _(st, srv, X, Y):
        leader(st, srv, X, Y)
        return msg(srv, abi.MSG_CONSISTENT_QUERY)
    return out


def build_rounds(engine, O, G, N, X, Y):
    """One-tick rounds over G x N servers: [(start state, messages in bucket order, decisions, rpcs, state after)];
    scenario k of a round sits on server k, the list repeats until the servers are used up (at most one full pass when
    it is longer than a round)."""
    sc = scenarios(N)
    S = G * N
    n_rounds = -(-len(sc) // S)
    rounds = []
    for r in range(n_rounds):
        st = abi.empty_server_states(G, N)
        msgs = []
        for srv in range(S):
            k = r * S + srv if n_rounds > 1 else srv
            if n_rounds > 1 and k >= len(sc):
                follower(st, srv, N, X, Y)
                continue
            msgs.append(sc[k % len(sc)][1](st, srv, X, Y))
        msgs = in_bucket_order(engine, np.array(msgs, dtype=abi.MSG_DTYPE), N)
        cpu = O.Oracle(G, N, max_runs=16)
        cpu.set_state(0, st)
        d, rp = cpu.step(msgs)
        rounds.append((st, msgs, d.copy(), rp.copy(), cpu.get_state()))
        cpu.close()
    return rounds


def check_coverage(rounds, tag, mixed_slices):
    seen = {}
    for _, _, dec, _, _ in rounds:
        for r in dec:
            for row in rows_of(r):
                seen[row] = seen.get(row, 0) + 1
    missing = sorted(REACHABLE - set(seen))
    assert not missing, f"{tag}: rows that no decision of the checker landed on: {missing}\n seen: {seen}"
    if mixed_slices:
        # a slice of 64 consecutive records that holds a record of a new form (or a flag set new to its form), one of a
        # form of minor 0 and a full one
        def cls(r):
            if compact_ref(r) is None:
                return "full"
            old = form_of(r) in ("wrote", "confirmed", "counted") and not int(r["flags"]) & ~PLAIN & CHANGE and \
                int(r["kind"]) in (abi.MSG_AER, abi.MSG_WRITTEN, abi.MSG_AER_REPLY) and \
                not (form_of(r) == "counted" and int(r["kind"]) == abi.MSG_AER)
            return "old" if old else "new"
        dec = rounds[0][2]
        mixed = [i for i in range(0, len(dec), 64) if {cls(r) for r in dec[i:i + 64]} == {"full", "old", "new"}]
        assert mixed, f"{tag}: no slice of 64 records mixes new-form, old-form and full records"


def assert_raw_stream(tag, raw: np.ndarray, msgs, want):
    """One tick's slots of a device-resident decision stream (uint8[n_slots, 64], filled with 0xEE before the launch):
    expanded = the checker's, RGB_F_COMPACT exactly where compact_ref fits and then compact_ref's 32 bytes, the half a
    compact record does not own still 0xEE -- and so is every slot behind the tick."""
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
            assert np.all(raw[i, 32:] == 0xEE), f"{where}: the upper half of a compact record was written"
        assert got[i].tobytes() == want[i].tobytes(), f"{where}:\n got ={got[i]}\n want={want[i]}"
    assert np.all(raw[n:] == 0xEE), f"{tag}: a slot behind the tick's {n} records was written"


def settle(on_gpu):
    """The buffers' fills and copies (torch's stream) have landed before the engine's own stream is given work on them."""
    if on_gpu:
        import torch
        torch.cuda.synchronize()


def check_forms(engine, O, G, N, X, Y, on_gpu, trains_only=False):
    import fuzz
    tag0 = f"{G} x {N}, indexes from {X:#x}, terms from {Y:#x}"
    rounds = build_rounds(engine, O, G, N, X, Y)
    check_coverage(rounds, tag0, mixed_slices=trains_only)            # before anything touches an engine
    S, per = G * N, max(N - 1, 1)
    tb, rs = S * 64, S * per * 56
    with engine.RaGpuBatch(G, N, max_runs=16, ring_slots=2, ring_capacity=max(1024, S)) as eng:
        for r, (st0, msgs, want, want_rp, st1) in enumerate(rounds):
            n = len(msgs)
            counts = np.array([n], dtype=np.uint32)
            kinds = np.bincount(msgs["kind"], minlength=abi.N_KINDS).astype(np.uint32).reshape(1, -1)
            buckets = np.bincount(engine.train_bucket(msgs["kind"], msgs["flags"], msgs["server"], N),
                                  minlength=engine.TRAIN_BUCKETS).astype(np.uint32).reshape(1, -1)
            dmsgs = Buf(tb, on_gpu)
            dmsgs.put(0, msgs.tobytes())
            rp_want = fuzz.sort_rpcs(want_rp).copy()
            rp_want["msg_index"] = 0

            def verify(tag, ddec, drpc):
                eng.synchronize()
                assert_raw_stream(tag, ddec.host()[:tb].reshape(S, 64), msgs, want)
                assert rpc_slots(drpc.host()[:rs], want, per).tobytes() == rp_want.tobytes(), tag + ": rpc records"
                assert_state_equal(tag, eng.get_state(), st1)

            if not trains_only:
                for name, kc in (("generic kernel", None), ("class kernels", kinds)):
                    eng.set_state(0, st0)
                    ddec, drpc = Buf(tb, on_gpu, 0xEE), Buf(rs, on_gpu)
                    settle(on_gpu)
                    eng.run_ticks_device(dmsgs.ptr, S, 1, ddec.ptr, drpc.ptr, tick_counts=counts, kind_counts=kc)
                    verify(f"{tag0}, round {r}, {name}", ddec, drpc)
            # both train forms: the host's plan (dealt), the plan built on the device (persistent)
            dbc = Buf(engine.TRAIN_BUCKETS * 4, on_gpu)
            dbc.put(0, buckets.tobytes())
            settle(on_gpu)
            for name in ("train, host plan", "train, device plan"):
                if name.endswith("host plan"):
                    plan = eng.train_plan(buckets)
                else:
                    plan = engine.TrainPlan(eng, None, device_ticks=1)
                    plan.build_device(0, 1, dbc.ptr)
                eng.set_state(0, st0)
                stamps, ddec, drpc = Buf(S, on_gpu), Buf(tb, on_gpu, 0xEE), Buf(rs, on_gpu)
                settle(on_gpu)
                eng.train_stamp_device(dmsgs.ptr, stamps.ptr, S, counts)
                eng.train_run_device(plan, 0, 1, dmsgs.ptr, stamps.ptr, S, ddec.ptr, drpc.ptr, rpc_ring=1)
                eng.synchronize()
                assert eng.train_status()[0] == 0
                verify(f"{tag0}, round {r}, {name} ({eng.train_form()})", ddec, drpc)
                plan.close()
            if trains_only:
                continue
            # the host paths: rgb_results_kernel expands on the device
            for name, step in (("rgb_submit", eng.step), ("rgb_submit_raw", lambda m: eng.step_raw(m, max_rounds=1))):
                eng.set_state(0, st0)
                tag = f"{tag0}, round {r}, {name}"
                dg, rg = step(msgs)
                assert len(dg) == len(want)
                for i in np.flatnonzero((dg.view(np.uint8).reshape(-1, 64) != want.view(np.uint8).reshape(-1, 64)).any(axis=1))[:1]:
                    raise AssertionError(f"{tag}: record {i} msg={msgs[i]}\n got ={dg[i]}\n want={want[i]}")
                assert fuzz.sort_rpcs(rg.copy()).tobytes() == fuzz.sort_rpcs(want_rp).tobytes(), tag + ": rpc records"
                assert_state_equal(tag, eng.get_state(), st1)


def check_closed_loop(engine, O, on_gpu, G=64, N=5, T=32, seed=0x5EED0003):
    """The load generator's ticks through the class kernel, the checker beside it."""
    from ra_amd import workload as W
    S, per = G * N, N - 1
    tb = S * 64
    st0 = W.initial_states(G, N, seed)
    cpu = O.Oracle(G, N, max_runs=16)
    cpu.set_state(0, st0)
    n_compact = n_new = 0
    with engine.RaGpuBatch(G, N, max_runs=16, ring_slots=1, ring_capacity=1024) as eng:
        eng.set_state(0, st0)
        dm, dd, dr, dn = Buf(tb, on_gpu), Buf(tb, on_gpu, 0xEE), Buf(S * per * 56, on_gpu), Buf(16, on_gpu)
        settle(on_gpu)
        for t in range(T):
            eng.synth_tick_buckets_device(seed, t, dm.ptr, 0, dn.ptr, 0)
            eng.synchronize()
            n = int(dn.host()[:4].view(np.uint32)[0])
            msgs = dm.host()[:n * 64].view(abi.MSG_DTYPE).copy()
            want, _ = cpu.step(msgs)
            eng.synth_apply_tick_device(dm.ptr, S, dd.ptr, dr.ptr)
            eng.synchronize()
            raw = dd.host()[:n * 64].view(abi.DECISION_DTYPE)
            got = abi.expand_decisions(raw)
            forms = abi.compact_forms(want)
            assert np.array_equal((raw["flags"] & abi.F_COMPACT) != 0, forms != 0), f"tick {t}: RGB_F_COMPACT against abi.compact_forms"
            for i in np.flatnonzero((got.view(np.uint8).reshape(-1, 64) != want.view(np.uint8).reshape(-1, 64)).any(axis=1))[:1]:
                raise AssertionError(f"tick {t}: record {i} msg={msgs[i]}\n got ={got[i]}\n want={want[i]}")
            n_compact += int((forms != 0).sum())
            n_new += sum(1 for r in want[forms != 0] if form_of(r) in NEW_FORMS or
                         int(r["kind"]) not in (abi.MSG_AER, abi.MSG_WRITTEN, abi.MSG_AER_REPLY))
        assert_state_equal("closed loop", eng.get_state(), cpu.get_state())
    cpu.close()
    assert n_compact > 0 and n_new > 0, "the closed loop produced no record of a new form"


# small values (zero anchors lie near); indexes and terms above 2^63; both as high as the contract lets them be (every
# value of every scenario below 2^64 - 2^16, fuzz.WIDE_LIMIT: RGB_UNDEF's neighbourhood is no index)
GROUND = [(0, 0), (2**63 - 1000, 2**63 - 21), (2**64 - 2**16 - 110_000, 2**64 - 2**16 - 400)]


@pytest.mark.parametrize("index_base,term_base", GROUND)
def test_forms_on_the_block_emulation(emulated_engine, oracle_lib, index_base, term_base):
    check_forms(emulated_engine, oracle_lib, 8, 5, index_base, term_base, False)


def test_train_slices_on_the_block_emulation(emulated_engine, oracle_lib):
    check_forms(emulated_engine, oracle_lib, 260, 5, 0, 0, False, trains_only=True)


def test_closed_loop_on_the_block_emulation(emulated_engine, oracle_lib):
    check_closed_loop(emulated_engine, oracle_lib, False)


@pytest.mark.gpu
@pytest.mark.parametrize("index_base,term_base", GROUND)
def test_gpu_forms(gpu_engine, oracle_lib, index_base, term_base):
    check_forms(gpu_engine, oracle_lib, 8, 5, index_base, term_base, True)


@pytest.mark.gpu
def test_gpu_train_slices(gpu_engine, oracle_lib):
    check_forms(gpu_engine, oracle_lib, 260, 5, 0, 0, True, trains_only=True)


@pytest.mark.gpu
def test_gpu_closed_loop(gpu_engine, oracle_lib):
    check_closed_loop(gpu_engine, oracle_lib, True)
