"""segment_read/5 of the Erlang NIF shim (ra_amd/csrc/ra_gpu_batch_nif.c) executed on the mock BEAM of
tests/native/mock_beam, linked to the CPU-emulated library, under a Python twin of the wrappers
ra_gpu_batch:segment_read_plan/3 and segment_term_query_batch/2 (erlang/ra_gpu_batch.erl, which no OTP here can run):
the twin builds the same binaries, calls the NIF and turns RowsBin / ResultsBin / OutBin into the same per-file answers.
Answers against ref_parse of tests/test_segment_compact.py (src/ra_log_segment.erl:375-598, 652-689, 1057-1075)."""
import os
import re
import struct
import zlib

import numpy as np

from test_nif_shim_mock_beam import beam, ROOT          # noqa: F401  (the fixture that builds and loads the shim)
from test_segment_compact import R, make_source, ref_parse, source_of

UNDEF = (1 << 64) - 1


# ---- the twin: erlang/ra_gpu_batch.erl, function by function

def read_plan_bins(plan):
    sources, files, req, off, first = b"", b"", b"", 0, 0
    for file_bin, idxs in plan:
        sources += struct.pack("<QQIIQ", off, len(file_bin), first, len(idxs), 0)
        files += file_bin
        req += b"".join(struct.pack("<Q", i) for i in idxs)
        off, first = off + len(file_bin), first + len(idxs)
    return sources, files, req


def read_plan_answers(plan, results_bin, rows_bin, answer):
    out, first = [], 0
    for k, (_file_bin, idxs) in enumerate(plan):
        st, n_read, idx = struct.unpack("<IIQ", results_bin[32 * k:32 * k + 16])
        out.append(answer(st, n_read, idx, rows_bin[32 * first:32 * (first + len(idxs))]))
        first += len(idxs)
    assert len(results_bin) == 32 * len(plan)
    return out


def segment_read_plan(beam, ctx, plan, opts):           # noqa: F811
    flags = 1 if opts.get("validate", False) else 0
    strategy = opts.get("strategy", "error")
    sources, files, req = read_plan_bins(plan)
    got = beam.call("segment_read", ctx, sources, files, req, flags)
    if got[0] != "ok":
        return got
    _, rows_bin, results_bin, out = got

    def entries(rows):
        return [(idx, term, out[off:off + ln]) for idx, term, off, ln, _crc in struct.iter_unpack("<QQQII", rows)]

    def answer(st, n_read, idx, rows):
        if st == 0:
            return ("ok", entries(rows))
        if st == 1 and strategy == "return":
            return ("ok", entries(rows[:32 * n_read]))
        return ("error", {1: ("missing_key", idx), 2: ("read_error", idx), 3: ("crc_check_failure", idx), 4: "bad_segment"}[st])
    return ("ok", read_plan_answers(plan, results_bin, rows_bin, answer))


def segment_term_query_batch(beam, ctx, plan):          # noqa: F811
    sources, files, req = read_plan_bins(plan)
    got = beam.call("segment_read", ctx, sources, files, req, 2)
    if got[0] != "ok":
        return got
    _, rows_bin, results_bin, out = got
    assert out == b""

    def answer(st, _n_read, _idx, rows):
        if st == 4:
            return ("error", "bad_segment")
        return ("ok", [None if off == UNDEF else term for _i, term, off, _l, _c in struct.iter_unpack("<QQQII", rows)])
    return ("ok", read_plan_answers(plan, results_bin, rows_bin, answer))


# ---- the tests

def test_segment_read_nif_and_the_wrappers_twin(beam):  # noqa: F811
    ok, ctx = beam.call("open", 0, 16, 2, 256)
    assert ok == "ok"
    rng = np.random.default_rng(36)
    a = source_of(rng, [1, 2, 3, 4, 5, 6, 3, 4, 7, 8, 9])                 # 5 and 6 went with the backwards step
    b = make_source([R(8 + j, 5, bytes([j]) * (40 * j)) for j in range(12)], max_count=20, version=1)
    ia, ib = ref_parse(a), ref_parse(b)

    def entry(f, index, i):
        term, pos, ln, _ = index[i]
        return (i, term, f[pos:pos + ln])

    # one good plan: two files, any order, an index twice
    plan = [(a, [9, 1, 4, 4, 7]), (b, list(range(19, 7, -1)))]
    want = [("ok", [entry(a, ia, i) for i in plan[0][1]]), ("ok", [entry(b, ib, i) for i in plan[1][1]])]
    for opts in ({}, {"validate": True}, {"strategy": "return"}):
        assert segment_read_plan(beam, ctx, plan, opts) == ("ok", want)

    # a missing key in one file, with and without strategy => return: the other file's answer stays
    plan = [(a, [1, 2, 5, 7]), (b, [8, 9])]
    good_b = ("ok", [entry(b, ib, 8), entry(b, ib, 9)])
    assert segment_read_plan(beam, ctx, plan, {}) == ("ok", [("error", ("missing_key", 5)), good_b])
    assert segment_read_plan(beam, ctx, plan, {"strategy": "return"}) == \
        ("ok", [("ok", [entry(a, ia, 1), entry(a, ia, 2)]), good_b])

    # a damaged payload: seen with validate only; a payload outside its file; a file that is no segment
    hurt = bytearray(b); hurt[ib[10][1]] ^= 1
    plan = [(bytes(hurt), [9, 10, 11]), (a, [1]), (b[:ib[19][1] + 3], [18, 19]), (b"RASX" + a[4:], [1])]
    assert zlib.crc32(bytes(hurt)[ib[10][1]:][:ib[10][2]]) != ib[10][3]
    got = segment_read_plan(beam, ctx, plan, {"validate": True})
    assert got == ("ok", [("error", ("crc_check_failure", 10)), ("ok", [entry(a, ia, 1)]), ("error", ("read_error", 19)),
                          ("error", "bad_segment")])
    assert segment_read_plan(beam, ctx, plan, {})[1][0] == ("ok", [entry(bytes(hurt), ib, i) for i in (9, 10, 11)])

    # one term-query batch
    plan = [(a, [9, 5, 1, 100]), (b, [19, 8]), (b"RASX", [1]), (a, [])]
    assert segment_term_query_batch(beam, ctx, plan) == \
        ("ok", [("ok", [ia[9][0], None, ia[1][0], None]), ("ok", [5, 5]), ("error", "bad_segment"), ("ok", [])])
    assert segment_read_plan(beam, ctx, [], {}) == ("ok", [])

    # binaries of the wrong size, arguments of the wrong kind; malformed contents are the library's {error, invalid}
    sources, files, req = read_plan_bins([(a, [1, 2]), (b, [8])])
    assert beam.call("segment_read", ctx, sources, files, req, 0)[0] == "ok"
    assert beam.call("segment_read", ctx, sources[:-1], files, req, 0) == "badarg"
    assert beam.call("segment_read", ctx, sources, files, req + b"\0", 0) == "badarg"
    assert beam.call("segment_read", ctx, sources, 7, req, 0) == "badarg"
    assert beam.call("segment_read", ctx, sources, files, req, 1 << 32) == "badarg"
    assert beam.call("segment_read", ctx, sources, files, req, 4) == ("error", "invalid")
    assert beam.call("segment_read", ctx, sources, files, req, 3) == ("error", "invalid")
    assert beam.call("segment_read", ctx, sources, files[:-1], req, 0) == ("error", "invalid")       # a source outside
    assert beam.call("segment_read", ctx, sources, files, req[:-8], 0) == ("error", "invalid")        # a slice outside
    beam.L.mock_gc_resource_term(ctx.t)


def test_segment_read_nif_is_dirty_and_matches_the_erlang_stub(beam):               # noqa: F811
    src = open(os.path.join(ROOT, "erlang", "ra_gpu_batch.erl")).read()
    stubs = dict(re.findall(r"^(\w+)\(([^)]*)\)\s*->\s*erlang:nif_error\(not_loaded\)\.", src, flags=re.M))
    assert len([x for x in stubs["segment_read"].split(",") if x.strip()]) == 5
    assert beam.L.mock_func_flags(b"segment_read", 5) == 2, "segment_read: dirty IO-bound, as wal_frame"
    assert "segment_read/5, segment_read_plan/3, segment_term_query_batch/2" in src  # exported
    assert "NOT COMPILED OR RUN" in src
