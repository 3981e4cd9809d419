"""segment_compact_plan/7 and segment_compact_groups/7 of the Erlang NIF shim (ra_amd/csrc/ra_gpu_batch_nif.c) executed
on the mock BEAM of tests/native/mock_beam, linked to the CPU-emulated library: the binary layouts and the answers
against the Python binding (engine.major_compaction_plan, segment_compact_groups) and the referees of
tests/test_segment_compact_groups.py."""
import os
import re
import struct

import numpy as np

from ra_amd import abi
from test_nif_shim_mock_beam import beam, ROOT          # noqa: F401  (the fixture that builds and loads the shim)
from test_segment_compact import ref_compact
from test_segment_compact_groups import extra_plan_cases, plan_members, ref_plan, suite_cases

ROW = np.dtype([("num_live", "<u8"), ("live_first", "<u4"), ("live_n", "<u4"), ("flags", "<u4"), ("group", "<u4"),
                ("status", "<u4"), ("_pad", "<u4")])


def test_segment_compact_groups_nifs(beam, emulated_engine):          # noqa: F811
    ok, ctx = beam.call("open", 0, 16, 2, 256)
    assert ok == "ok"
    conf, cases = suite_cases()
    cases = [c for c in cases if c["kind"] == "major"] + extra_plan_cases()
    buf, members, kept = plan_members(cases)
    mem = np.zeros(len(members), dtype=abi.SEG_MEMBER_DTYPE)
    segrefs, live = b"", []
    n_refs = 0
    for m, (refs, pairs) in enumerate(members):
        mem[m] = (n_refs, len(refs), len(live), len(pairs))
        segrefs += b"".join(struct.pack("<QQQQ", off, n, r[0], r[1]) for off, n, r in refs)
        n_refs += len(refs)
        live += pairs
    live_bin = np.array(live, dtype=np.uint64).reshape(-1, 2).tobytes()
    ok, rows_bin, groups_bin, live_out_bin = beam.call("segment_compact_plan", ctx, mem.tobytes(), segrefs, buf.tobytes(),
                                                       live_bin, conf["max_count"], conf["max_size"])
    assert ok == "ok"
    rows = np.frombuffer(rows_bin, dtype=ROW)
    groups = np.frombuffer(groups_bin, dtype=abi.SEG_GROUP_DTYPE)
    live_out = np.frombuffer(live_out_bin, dtype=np.uint64).reshape(-1, 2)
    assert len(rows) == n_refs

    # against the Python binding: the same groups, layout and selections
    eng = emulated_engine.RaGpuBatch(1, 1)
    try:
        plan = eng.major_compaction_plan(members, buf, conf["max_count"], conf["max_size"])
        assert groups.tobytes() == plan["groups"].tobytes() and live_out.tobytes() == plan["live"].tobytes()
        # ... and against the referees, member by member
        sources, g = [], 0
        for m, (files, ranges, compactable, live_m) in enumerate(kept):
            want_groups, dele = ref_plan(files, ranges, compactable, live_m, conf)
            base = int(mem["segref_first"][m])
            mine = rows[base:base + len(compactable)]
            assert [compactable[k] for k in range(len(mine)) if int(mine["flags"][k]) & 1][::-1] == dele
            assert all(int(s) == abi.SEG_TAKE_OK for s in mine["status"])
            for grp in want_groups:
                ks = [k for k in range(len(mine)) if int(mine["group"][k]) == g][::-1]             # oldest first
                assert [compactable[k] for k in ks] == grp, cases[m]["name"]
                for k in ks:
                    off, n, _ = members[m][0][k]
                    sources.append((off, n, int(mine["live_first"][k]), int(mine["live_n"][k]), 0))
                g += 1
        assert g == len(groups)
        sources = np.array(sources, dtype=abi.SEG_SOURCE_DTYPE)
        assert sources.tobytes() == plan["sources"].tobytes()
        # The Erlang wrapper major_compaction_batch builds SourcesBin from RowsBin alone: every row that has a group,
        # sorted by (group, -row number) -- lists:sort/1 on {Group, -K, ...} -- which has to be the order GroupsBin's
        # src_first / src_n count in: group by group, a member's LAST segref (its oldest file) first.  Restated here
        # over what the NIF returned; sorting by the group alone (stable) would leave every group newest first.
        offs = [(off, n) for refs, _ in members for off, n, _ in refs]
        tagged = sorted((int(rows["group"][k]), -k) for k in range(len(rows)) if int(rows["group"][k]) != abi.SEG_GROUP_NONE)
        wrapper = np.array([(offs[-nk][0], offs[-nk][1], int(rows["live_first"][-nk]), int(rows["live_n"][-nk]), 0)
                            for _, nk in tagged], dtype=abi.SEG_SOURCE_DTYPE)
        assert wrapper.tobytes() == plan["sources"].tobytes()
        assert any(int(g["src_n"]) > 1 for g in groups), "no group of two files: the order within a group is not exercised"
        stable = sorted(((int(rows["group"][k]), k) for k in range(len(rows)) if int(rows["group"][k]) != abi.SEG_GROUP_NONE),
                        key=lambda t: t[0])
        assert [k for _, k in stable] != [-nk for _, nk in tagged], "ascending rows within a group would be newest first"
        erl = open(os.path.join(ROOT, "erlang", "ra_gpu_batch.erl")).read()
        assert "lists:sort([{Group, -K, Off, Len, LiveFirst, LiveN}" in erl and "keysort(1, [{Group, -K" not in erl

        for flags in (0, abi.SEG_COMPACT_VERIFY):
            ok, res_bin, out_bin = beam.call("segment_compact_groups", ctx, groups_bin, sources.tobytes(), buf.tobytes(),
                                             live_out_bin, conf["max_size"], flags)
            assert ok == "ok"
            res = np.frombuffer(res_bin, dtype=abi.SEG_COMPACT_RESULT_DTYPE)
            want_res, images = eng.segment_compact_groups(groups, sources, buf, live_out, conf["max_size"], flags)
            assert res.tobytes() == want_res.tobytes() and len(out_bin) == plan["out_bytes"]
            for k in range(len(groups)):
                off = int(groups["out_offset"][k])
                assert int(res["status"][k]) == abi.SEG_COMPACT_OK
                assert out_bin[off:off + int(res["file_bytes"][k])] == images[k].tobytes()
        # the first group once more against the sequential referee
        files, ranges, compactable, live_m = kept[0]
        grp = ref_plan(files, ranges, compactable, live_m, conf)[0][0]
        lives = [[(max(a, ranges[k][0]), min(b, ranges[k][1])) for a, b in live_m if a <= ranges[k][1] and b >= ranges[k][0]]
                 for k in grp]
        want = ref_compact([files[k] for k in grp], lives, conf["max_size"])
        assert out_bin[:len(want)] == want

        # a failing group leaves the others: damage the header of the second group's first file
        bad = bytearray(buf.tobytes())
        first = int(sources["offset"][int(groups["src_first"][1])])
        bad[first] = ord("X")
        ok, res_bin, out_bin2 = beam.call("segment_compact_groups", ctx, groups_bin, sources.tobytes(), bytes(bad),
                                          live_out_bin, conf["max_size"], 0)
        res = np.frombuffer(res_bin, dtype=abi.SEG_COMPACT_RESULT_DTYPE)
        assert ok == "ok" and [int(s) for s in res["status"]] == [0, abi.SEG_COMPACT_BAD_SOURCE] + [0] * (len(groups) - 2)
        lo, hi = int(groups["out_offset"][1]), int(groups["out_offset"][1]) + int(groups["out_bytes"][1])
        assert out_bin2[:lo] == out_bin[:lo] and out_bin2[hi:] == out_bin[hi:] and out_bin2[lo:hi] == bytes(hi - lo)
    finally:
        eng.close()

    # binaries of the wrong size, arguments of the wrong kind; malformed contents are the library's {error, invalid}
    args = (mem.tobytes(), segrefs, buf.tobytes(), live_bin)
    assert beam.call("segment_compact_plan", ctx, args[0][:-1], *args[1:], 128, 128000) == "badarg"
    assert beam.call("segment_compact_plan", ctx, args[0], args[1][:-8], *args[2:], 128, 128000) == "badarg"
    assert beam.call("segment_compact_plan", ctx, *args[:3], args[3] + b"\0", 128, 128000) == "badarg"
    assert beam.call("segment_compact_plan", ctx, *args, "many", 128000) == "badarg"
    assert beam.call("segment_compact_plan", ctx, args[0], args[1][:-32], *args[2:], 128, 128000) == ("error", "invalid")
    assert beam.call("segment_compact_plan", ctx, *args[:2], args[2][:-3000], args[3], 128, 128000) == ("error", "invalid")
    cg = (groups_bin, sources.tobytes(), buf.tobytes(), live_out_bin)
    assert beam.call("segment_compact_groups", ctx, cg[0][:-1], *cg[1:], conf["max_size"], 0) == "badarg"
    assert beam.call("segment_compact_groups", ctx, cg[0], cg[1][:-1], *cg[2:], conf["max_size"], 0) == "badarg"
    assert beam.call("segment_compact_groups", ctx, *cg, conf["max_size"], 1 << 32) == "badarg"
    assert beam.call("segment_compact_groups", ctx, *cg, conf["max_size"], 2) == ("error", "invalid")
    assert beam.call("segment_compact_groups", ctx, cg[0], cg[1][:-32], *cg[2:], conf["max_size"], 0) == ("error", "invalid")
    overlap = groups.copy(); overlap["out_offset"][1] = overlap["out_offset"][0]
    assert beam.call("segment_compact_groups", ctx, overlap.tobytes(), *cg[1:], conf["max_size"], 0) == ("error", "invalid")
    assert beam.call("segment_compact_groups", ctx, b"", b"", b"", b"", conf["max_size"], 0) == ("ok", b"", b"")
    beam.L.mock_gc_resource_term(ctx.t)


def test_segment_compact_groups_nifs_are_dirty_and_match_the_erlang_stub(beam):            # noqa: F811
    src = open(os.path.join(ROOT, "erlang", "ra_gpu_batch.erl")).read()
    stubs = dict(re.findall(r"^(\w+)\(([^)]*)\)\s*->\s*erlang:nif_error\(not_loaded\)\.", src, flags=re.M))
    for name, arity in (("segment_compact_plan", 7), ("segment_compact_groups", 7)):
        assert len([a for a in stubs[name].split(",") if a.strip()]) == arity
        assert beam.L.mock_func_flags(name.encode(), arity) == 2, f"{name}: dirty IO-bound, as wal_frame"
    assert "segment_compact_plan/7, segment_compact_groups/7, major_compaction_batch/4" in src      # exported
    assert "NOT COMPILED OR RUN" in src
