"""Major compaction for many members in one call: the plan helpers rgb_segment_compact_select / _take_groups /
_groups_bound and the batched copy rgb_segment_compact_groups* (include/ra_gpu_wal.h, "major compaction for many
members in one call"; ra_amd/csrc/rgb_segment.hip, rgb_segment_host.cpp).

Referees.  The copy: ref_compact of tests/test_segment_compact.py per group, and rgb_segment_compact* called for that
group alone through the same back end -- the batched call promises exactly that call's image and result row.  The plan:
two pure-Python functions written sequentially from the reference source, with lists and Erlang's control flow --
  ref_select       the fold of major_compaction/3   src/ra_log_segments.erl:745-761 (and of minor_compaction/2, :843-854)
                   over real ra_seq lists, handled by the seq_* restatements of tests/ra_log_model.py (expand / filter /
                   rebuild); the library clips pairs by binary search, the referee deliberately does not
  ref_take_groups  compaction_groups/3 + take_group/3   :901-950, with true float division and short-circuit `or`;
                   ZeroDivisionError where Erlang raises badarith
-- pinned to what the reference's own suite asserts (test/ra_log_segments_SUITE.erl: minor, major, major_max_size,
major_max_size_2; inputs and stated outcomes as data in tests/golden/ra_log_segments_suite_cases.json).

Every device check exists twice: on the CPU emulation of the same sources (-m "not gpu") and on the GPU."""
import ctypes
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from emu_schedule import PERMUTED_SCHEDULES, schedule
from ra_amd import abi
from ra_log_model import seq_expand, seq_floor, seq_from_list, seq_limit
from test_segment import Emu, Gpu, emu, gpu, first_diff                                  # noqa: F401  (fixtures)
from test_segment_compact import (CHUNK, R, device_compact, make_source, pack_group, precedence_group, ranges_of,
                                  ref_compact, ref_info, ref_parse, rnd_payloads, source_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL = -1
OK, MISSING, FULL, TRUNCATED, SPACE, CRC, BAD_SOURCE = range(7)
VERIFY = abi.SEG_COMPACT_VERIFY
MAX_SIZE = abi.SEG_MAX_SIZE_B
NONE = abi.SEG_GROUP_NONE
THREADS = 256                  # rgb_segment.hip: lanes of a workgroup of the copy; THREADS / width entries each
GUARD = 48
ROW_FIELDS = ("status", "n_entries", "file_bytes", "index", "source")


# ------------------------------------------------------------------------------------------ referees of the plan

def ref_select(segrefs, live):
    """segrefs: [(Start, End)] newest first; live: [(first, last)] or None (undefined).  -> (Compactable as
    [(segref ordinal, Seq as ascending indexes)] in the fold's final order -- oldest first --, Delete as ordinals in the
    fold's final order)."""
    live_seq = seq_from_list([i for a, b in (live or []) for i in range(a, b + 1)])
    comps, dele = [], []
    for k, (start, end) in enumerate(segrefs):
        if not live_seq or start > end:                      # in_range(_, []) / in_range(undefined, _)
            seq = []
        else:
            seq = seq_floor(start, seq_limit(end, live_seq))     # in_range/2 :227-229
        if seq == []:
            dele = [k] + dele
        else:
            comps = [(k, seq_expand(seq))] + comps
            live_seq = seq_limit(end, live_seq)
    return comps, dele


def _take_group(infos, conf, acc):
    """take_group/3: infos = [(info dict, num_live, tag)] -> (Group, RemInfos)"""
    while True:
        if not infos:
            return list(reversed(acc)), []
        e, rem = infos[0], infos[1:]
        info, num_live = e[0], e[1]
        all_data_sz = info["size"] - info["index_size"]
        if num_live / info["num_entries"] < 0.5 or info["live_size"] / all_data_sz < 0.5:
            if conf["max_count"] - num_live < 0 or conf["max_size"] - info["live_size"] < 0:
                if acc == []:
                    infos = rem
                    continue
                return list(reversed(acc)), infos
            conf = dict(max_count=conf["max_count"] - num_live, max_size=conf["max_size"] - info["live_size"])
            infos, acc = rem, [e] + acc
            continue
        if acc == []:
            infos = rem
            continue
        return list(reversed(acc)), rem


def ref_take_groups(infos, conf):
    """compaction_groups/3 -> [[tag]]; raises ZeroDivisionError where the reference raises badarith"""
    groups = []
    while infos:
        group, infos = _take_group(infos, conf, [])
        if group:
            groups = [group] + groups
    return [[e[2] for e in g] for g in reversed(groups)]


# ------------------------------------------------------------------------------------------ the plan helpers

def lib_select(engine, members):
    """members: [(segrefs, live or None)] -> per member (comps, dele) in ref_select's form, through the library"""
    mem = np.zeros(len(members), dtype=abi.SEG_MEMBER_DTYPE)
    segrefs, live = [], []
    for m, (refs, pairs) in enumerate(members):
        mem[m] = (len(segrefs), len(refs), len(live), len(pairs or []))
        segrefs += refs
        live += list(pairs or [])
    picks, out = engine.segment_compact_select(mem, segrefs, live)
    assert engine.segment_compact_select(mem, segrefs, live, sizing=True) == len(out)
    answers, at = [], 0
    for m, (refs, _) in enumerate(members):
        comps, dele = [], []
        for k in range(len(refs)):
            p = picks[int(mem["segref_first"][m]) + k]
            assert int(p["live_first"]) == at, "the selections are not back to back in segref order"
            at += int(p["live_n"])
            pairs = [(int(a), int(b)) for a, b in out[int(p["live_first"]):int(p["live_first"]) + int(p["live_n"])]]
            if int(p["flags"]) & abi.SEG_PICK_UNREFERENCED:
                assert not pairs and int(p["num_live"]) == 0
                dele = [k] + dele
            else:
                assert int(p["flags"]) == 0 and pairs
                assert int(p["num_live"]) == sum(b - a + 1 for a, b in pairs)
                comps = [(k, pairs)] + comps
        answers.append((comps, dele))
    assert at == len(out)
    return answers


def check_select(engine, members, what=""):
    got = lib_select(engine, members)
    for m, (refs, pairs) in enumerate(members):
        comps, dele = ref_select(refs, pairs)
        want = ([(k, ranges_of(idxs)) for k, idxs in comps], dele)
        assert got[m] == want, f"{what} member {m}: segrefs {refs} live {pairs}: {got[m]} != {want}"


def info_rows(rows):
    out = np.zeros(len(rows), dtype=abi.SEG_INFO_DTYPE)
    for i, r in enumerate(rows):
        for k in ("num_entries", "index_size", "size", "live_size"):
            out[k][i] = r[k]
    return out


def check_take_groups(engine, members, conf, what=""):
    """members: [[(info dict, num_live)]] oldest first"""
    take = np.zeros(len(members), dtype=abi.SEG_TAKE_MEMBER_DTYPE)
    flat = []
    for m, rows in enumerate(members):
        take[m] = (len(flat), len(rows), 0, 0)
        flat += rows
    took, group_of = engine.segment_compact_take_groups(take, info_rows([r[0] for r in flat]),
                                                        [r[1] for r in flat], conf["max_count"], conf["max_size"])
    for m, rows in enumerate(members):
        first = int(take["src_first"][m])
        mine = [int(g) for g in group_of[first:first + len(rows)]]
        try:
            want = ref_take_groups([(info, nl, j) for j, (info, nl) in enumerate(rows)], conf)
        except ZeroDivisionError:
            assert int(took["status"][m]) == abi.SEG_TAKE_BADARITH and int(took["n_groups"][m]) == 0, f"{what} member {m}"
            assert all(g == NONE for g in mine), f"{what} member {m}"
            continue
        assert int(took["status"][m]) == abi.SEG_TAKE_OK, f"{what} member {m}: {rows}"
        got = [[j for j, g in enumerate(mine) if g == k] for k in range(int(took["n_groups"][m]))]
        assert got == want, f"{what} member {m}: {rows} conf {conf}: {got} != {want}"
        assert all(g == NONE or g < len(want) for g in mine)


def I(num_entries, num_live, live_size=10, data=1000, index_size=8 + 32 * 128):
    return dict(num_entries=num_entries, index_size=index_size, size=index_size + data, live_size=live_size), num_live


def test_select_hand_cases(emulated_engine):
    eng = emulated_engine
    files = [(300, 399), (200, 299), (100, 199)]
    U = (1 << 64) - 1
    cases = [
        ("a pair that spans two files and one that spans three", files, [(150, 250), (290, 310)]),
        ("a pair that spans three files", files, [(120, 380)]),
        ("one pair covers everything and more", files, [(1, 1000)]),
        ("pairs that end and begin on the file edges", files, [(100, 199), (201, 298), (300, 300), (399, 399)]),
        ("an empty selection in the middle leaves the ceiling alone", files, [(110, 120), (350, 360)]),
        ("nothing live in the newest files", files, [(90, 105)]),
        ("all files unreferenced", files, [(1, 99), (400, 500)]),
        ("an undefined live list", files, None),
        ("an empty live list", files, []),
        ("no segrefs", [], [(1, 5)]),
        # ends that do not descend: a later segref reaches above an earlier one and meets the ceiling
        ("ascending ends", [(100, 199), (200, 299), (300, 399)], [(150, 350)]),
        ("an overlapping older segref", [(200, 299), (150, 320)], [(140, 330)]),
        ("equal ends", [(200, 299), (100, 299)], [(50, 400)]),
        ("an empty selection above, then a wide one: the ceiling stayed unbounded", [(500, 600), (100, 450)], [(120, 440)]),
        ("a segref with Start > End", [(300, 399), (250, 200), (100, 199)], [(100, 399)]),
        ("indexes across 2^32", [(1 << 32, (1 << 32) + 50), ((1 << 32) - 60, (1 << 32) - 1)],
         [((1 << 32) - 10, (1 << 32) + 10), ((1 << 32) + 40, (1 << 32) + 100)]),
        ("indexes near 2^64 - 1", [(U - 20, U), (U - 60, U - 21)], [(U - 50, U - 45), (U - 25, U - 15), (U - 3, U)]),
        ("the last index alone", [(U, U), (U - 5, U - 1)], [(U - 1, U)]),
    ]
    for name, refs, live in cases:
        check_select(eng, [(refs, live)], name)
    check_select(eng, [(refs, live) for _, refs, live in cases], "all hand cases as members of one call")
    # worked by hand: the pair 150-250 is cut at the file edge, and the second file sees only what the first left
    (comps, dele), = lib_select(eng, [(files, [(150, 250), (290, 310)])])
    assert comps == [(2, [(150, 199)]), (1, [(200, 250), (290, 299)]), (0, [(300, 310)])] and dele == []
    # one range of 2^64 indexes: ra_seq:length saturates
    mem = np.zeros(1, dtype=abi.SEG_MEMBER_DTYPE); mem[0] = (0, 1, 0, 1)
    picks, out = eng.segment_compact_select(mem, [(0, U)], [(0, U)])
    assert int(picks["num_live"][0]) == U and [tuple(int(x) for x in p) for p in out] == [(0, U)]


def test_select_random_members(emulated_engine):
    rng = np.random.default_rng(7100)
    members = []
    for _ in range(300):
        n_files = int(rng.integers(0, 7))
        edges = sorted(int(x) for x in rng.choice(np.arange(1, 400), size=2 * n_files, replace=False)) if n_files else []
        refs = [(edges[2 * k], edges[2 * k + 1]) for k in range(n_files)][::-1]              # newest first
        if n_files and rng.random() < 0.25:
            rng.shuffle(refs)                                # unordered input: whatever the fold gives
            refs = [tuple(int(x) for x in r) for r in refs]
        if n_files and rng.random() < 0.2:
            k = int(rng.integers(0, n_files))
            refs[k] = (refs[k][0], refs[k][1] + int(rng.integers(0, 80)))                    # overlaps a newer file
        idxs = [int(i) for i in np.flatnonzero(rng.random(420) < rng.choice([0.02, 0.3, 0.8]))]
        members.append((refs, ranges_of(idxs) if rng.random() > 0.05 else None))
    check_select(emulated_engine, members, "random")
    for m in members[:40]:
        check_select(emulated_engine, [m], "random, alone")


def test_select_refusals(emulated_engine):
    eng = emulated_engine

    def refused(mem_rows, segrefs, live):
        mem = np.zeros(len(mem_rows), dtype=abi.SEG_MEMBER_DTYPE)
        for i, r in enumerate(mem_rows):
            mem[i] = r
        with pytest.raises(eng.RgbError) as e:
            eng.segment_compact_select(mem, segrefs, live)
        assert e.value.code == E_INVAL
    refs, live = [(10, 20), (1, 9)], [(1, 3), (5, 9)]
    refused([(0, 3, 0, 2)], refs, live)                      # segref slice outside the list
    refused([(3, 0, 0, 2)], refs, live)
    refused([(0, 2, 1, 2)], refs, live)                      # live slice outside the list
    refused([(0, 2, 0xFFFFFFFF, 2)], refs, live)
    refused([(0, 2, 0, 2), (1, 1, 0, 2)], refs, live)        # segref slices overlap
    refused([(1, 1, 0, 2), (0, 1, 0, 2)], refs, live)        # ... or do not ascend
    refused([(0, 2, 0, 2)], refs, [(5, 9), (1, 3)])          # pairs not ascending
    refused([(0, 2, 0, 2)], refs, [(1, 3), (4, 9)])          # adjacent
    refused([(0, 2, 0, 1)], refs, [(3, 1)])                  # first > last
    # a cap that is too small writes nothing
    mem = np.zeros(1, dtype=abi.SEG_MEMBER_DTYPE); mem[0] = (0, 2, 0, 2)
    picks = np.full(2, 0, dtype=abi.SEG_PICK_DTYPE); picks.view(np.uint8)[:] = 0xEE
    out = np.full((4, 2), 0xEEEE, dtype=np.uint64)
    n = ctypes.c_uint32(0)
    sr, lv = np.array(refs, dtype=np.uint64), np.array([(1, 3), (5, 15)], dtype=np.uint64)
    rc = eng.lib().rgb_segment_compact_select(mem.ctypes.data, 1, sr.ctypes.data, 2, lv.ctypes.data, 2, picks.ctypes.data,
                                              out.ctypes.data, 2, ctypes.byref(n))
    assert rc == E_INVAL and np.all(picks.view(np.uint8) == 0xEE) and np.all(out == 0xEEEE)
    rc = eng.lib().rgb_segment_compact_select(mem.ctypes.data, 1, sr.ctypes.data, 2, lv.ctypes.data, 2, picks.ctypes.data,
                                              out.ctypes.data, 3, ctypes.byref(n))
    assert rc == 0 and n.value == 3 and out[:3].tolist() == [[10, 15], [1, 3], [5, 9]]


def test_take_groups_every_exit(emulated_engine):
    eng = emulated_engine
    conf = dict(max_count=128, max_size=128_000)
    live, dense, big = I(100, 10), I(100, 90, live_size=900), I(1000, 129)
    cases = [
        ("no sources", []),
        ("one compactable source", [live]),
        ("not compactable, nothing accumulated: skipped", [dense, live]),
        ("not compactable behind a group: the group closes and the source is dropped", [live, live, dense, live]),
        ("over the count with nothing accumulated: skipped", [big, live]),
        ("over the count behind a group: the group closes and the source stays", [I(100, 40), I(100, 45), I(100, 44), I(100, 3)]),
        ("exactly the count is not over", [I(300, 64), I(300, 64), I(300, 1)]),
        ("over the size behind a group", [I(100, 1, live_size=70_000), I(100, 1, live_size=58_000), I(100, 1, live_size=1)]),
        ("exactly the size is not over", [I(100, 1, live_size=100_000, data=10 ** 6), I(100, 1, live_size=28_000, data=10 ** 6)]),
        ("over the size with nothing accumulated", [I(100, 1, live_size=128_001, data=10 ** 6), live]),
        ("a source that stays is over the fresh budgets too: skipped then", [live, big, live]),
        ("compactable by size only", [I(100, 60, live_size=100, data=1000)]),
        ("budgets start again with every group", [I(100, 45), I(100, 45), I(100, 45), I(100, 45), I(100, 45)]),
        ("ratio exactly 0.5 on the count, below on the size", [I(4, 2, live_size=49, data=100)]),
        ("ratio exactly 0.5 on both", [I(4, 2, live_size=50, data=100), live]),
        ("ratio exactly 0.5 on the size, above on the count", [I(4, 3, live_size=50, data=100)]),
        ("one below 0.5 on the count", [I(5, 2, live_size=100, data=100)]),
        ("size below index_size", [(dict(num_entries=4, index_size=500, size=300, live_size=0), 4)]),
        ("badarith: no entries", [live, I(0, 0), live]),
        ("badarith: no entries although nothing is live", [I(0, 0, live_size=0, data=0)]),
        ("badarith: no data and the first test false", [I(4, 2, live_size=0, data=0)]),
        ("no data, but orelse never looks: the first test is true", [I(4, 1, live_size=0, data=0), live]),
        ("more live than entries", [I(10, 2 ** 40), live]),
    ]
    cases = [(n, [tuple(r) for r in rows]) for n, rows in cases]
    for name, rows in cases:
        check_take_groups(eng, [rows], conf, name)
    check_take_groups(eng, [rows for _, rows in cases], conf, "all cases as members of one call")   # a crash stays inside its member
    # worked by hand from take_group/3
    take = np.zeros(1, dtype=abi.SEG_TAKE_MEMBER_DTYPE); take[0] = (0, 4, 0, 0)
    rows = [I(100, 40), I(100, 45), I(100, 44), I(100, 3)]
    took, group_of = eng.segment_compact_take_groups(take, info_rows([r[0] for r in rows]), [r[1] for r in rows], 128, 128_000)
    assert int(took["n_groups"][0]) == 2 and group_of.tolist() == [0, 0, 1, 1]
    with pytest.raises(eng.RgbError):
        take[0] = (2, 3, 0, 0)
        eng.segment_compact_take_groups(take, info_rows([r[0] for r in rows]), [r[1] for r in rows], 128, 128_000)


def test_take_groups_random(emulated_engine):
    rng = np.random.default_rng(7200)
    for conf in (dict(max_count=20, max_size=500), dict(max_count=128, max_size=128_000), dict(max_count=0, max_size=0)):
        members = []
        for _ in range(150):
            rows = []
            for _ in range(int(rng.integers(0, 9))):
                ents = int(rng.integers(0, 24)) if rng.random() < 0.9 else 0
                data = int(rng.choice([0, 1, 2, 100, 400, 1000]))
                rows.append((dict(num_entries=ents, index_size=520, size=520 + data, live_size=int(rng.integers(0, data + 2))),
                             int(rng.integers(0, ents + 3))))
            members.append(rows)
        check_take_groups(emulated_engine, members, conf, f"random, conf {conf}")


# ------------------------------------------------------------------------------------------ the suite's cases, end to end

def suite_cases():
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "ra_log_segments_suite_cases.json")))
    return doc["conf"], doc["cases"]


def suite_member(case):
    """The segment files the case's appends leave (append_to_segment: a successor when MaxCount records are in), its
    compactable segrefs newest first (compactable_segrefs/2 :857-881: never the newest file, End =< SnapIdx) and the
    live pairs."""
    mc, segs = case["segment_max_count"], []
    for block in case["entries"]:
        for idx in range(block["first"], block["last"] + 1):
            if not segs or len(segs[-1]) == mc:
                segs.append([])
            segs[-1].append(R(idx, 1, bytes([idx % 251]) * block["payload_bytes"]))
    files = [make_source(recs, max_count=mc) for recs in segs]
    ranges = [(recs[0]["idx"], recs[-1]["idx"]) for recs in segs]
    assert len(files) == case["segrefs_before"]
    compactable = [k for k in range(len(files) - 1) if ranges[k][1] <= case["snap_idx"]][::-1] if len(files) > 1 else []
    live = ranges_of(i for first, last, step in case["live"] for i in range(first, last + 1, step))
    return files, ranges, compactable, live


def ref_plan(files, ranges, compactable, live, conf):
    """major_compaction/3 up to the groups, by the referees: -> (groups as lists of file ordinals, Delete)"""
    comps, dele = ref_select([ranges[k] for k in compactable], live)
    infos = [(ref_info(files[compactable[k]], ranges_of(idxs)), len(idxs), compactable[k]) for k, idxs in comps]
    return ref_take_groups(infos, conf), [compactable[k] for k in dele]


def test_referees_on_the_suite_cases():
    conf, cases = suite_cases()
    seen = {}
    for case in cases:
        files, ranges, compactable, live = suite_member(case)
        if "segment_ranges" in case:
            assert [list(r) for r in ranges] == case["segment_ranges"]
        if case["kind"] == "minor":
            _, dele = ref_select([ranges[k] for k in compactable], live)
            assert len(files) - len(dele) == case["segrefs_after"], case["name"]
            seen[case["name"]] = [compactable[k] for k in dele]
            continue
        groups, dele = ref_plan(files, ranges, compactable, live, conf)
        linked = sum(len(g) - 1 for g in groups)
        assert len(files) - len(dele) - linked == case["segrefs_after"], case["name"]
        if "symlinks_after" in case:
            assert linked == case["symlinks_after"] and len(files) - len(dele) == case["files_after"], case["name"]
        if "first_file_num_entries_after" in case:
            assert groups[0][0] == 0
            lives = [[p for p in live if ranges[k][0] <= p[0] and p[1] <= ranges[k][1]] for k in groups[0]]
            image = ref_compact([files[k] for k in groups[0]], lives)
            assert len(ref_parse(image)) == case["first_file_num_entries_after"]
        seen[case["name"]] = groups
    # the groupings behind those counts, worked from take_group/3 by hand (see the budgets in the golden file's conf)
    assert seen == {"minor": [1], "minor_purge": [0, 1], "major": [[0, 1], [2], [4]], "major_max_size": [[0, 1], [2]],
                    "major_max_size_2": [[0]]}


def plan_members(cases):
    """The members of one major_compaction_plan call: every case's files in ONE buffer"""
    buf, members, kept = bytearray(), [], []
    for case in cases:
        files, ranges, compactable, live = suite_member(case)
        refs = []
        for k in compactable:
            buf += b"\xa5" * (1 + k)
            refs.append((len(buf), len(files[k]), ranges[k]))
            buf += files[k]
        members.append((refs, live))
        kept.append((files, ranges, compactable, live))
    return np.frombuffer(bytes(buf), dtype=np.uint8).copy(), members, kept


def extra_plan_cases():
    """members beyond the suite's: trimmed and overwritten records (num_entries above the indexes), a file skipped in
    the middle of the candidates, nothing live at all, a single candidate"""
    rng = np.random.default_rng(7300)
    def case(name, blocks, live, snap, mc=32):
        return dict(name=name, segment_max_count=mc, entries=blocks, kind="major", snap_idx=snap, live=live,
                    segrefs_before=sum(-(-(b["last"] - b["first"] + 1) // mc) for b in blocks))
    return [case("sparse", [dict(first=1, last=160, payload_bytes=int(rng.integers(0, 40)))], [[1, 160, 7]], 160),
            case("dense middle", [dict(first=1, last=160, payload_bytes=9)], [[1, 32, 5], [33, 64, 1], [65, 128, 6]], 128),
            case("nothing live", [dict(first=1, last=96, payload_bytes=3)], [], 96),
            case("one candidate", [dict(first=1, last=40, payload_bytes=17)], [[2, 30, 9]], 40)]


def check_plan(be):
    conf, cases = suite_cases()
    cases = [c for c in cases if c["kind"] == "major"] + extra_plan_cases()
    buf, members, kept = plan_members(cases)
    plan = be.eng.major_compaction_plan(members, buf, conf["max_count"], conf["max_size"])
    g = 0
    specs = []
    for m, (files, ranges, compactable, live) in enumerate(kept):
        groups, dele = ref_plan(files, ranges, compactable, live, conf)
        assert plan["status"][m] == abi.SEG_TAKE_OK
        assert [compactable[k] for k in plan["unreferenced"][m]] == dele, cases[m]["name"]
        mine = [(mm, [compactable[k] for k in ks]) for mm, ks in plan["group_files"] if mm == m]
        assert [ks for _, ks in mine] == groups, f"{cases[m]['name']}: {mine} != {groups}"
        in_groups = {k for grp in groups for k in grp}
        assert sorted(compactable[k] for k in plan["skipped"][m]) == sorted(set(compactable) - set(dele) - in_groups)
        for grp in groups:
            row = plan["groups"][g]
            srcs = plan["sources"][int(row["src_first"]):int(row["src_first"]) + int(row["src_n"])]
            lives = [[(int(a), int(b)) for a, b in plan["live"][int(s["live_first"]):int(s["live_first"]) + int(s["live_n"])]]
                     for s in srcs]
            assert lives == [[(max(a, ranges[k][0]), min(b, ranges[k][1])) for a, b in live
                              if a <= ranges[k][1] and b >= ranges[k][0]] for k in grp]
            assert int(plan["max_counts"][g]) == sum(b - a + 1 for l in lives for a, b in l)
            specs.append(([files[k] for k in grp], lives))
            g += 1
    assert g == len(plan["groups"]) and plan["out_bytes"] == sum(int(x) for x in plan["groups"]["out_bytes"])
    # ... and the copy of exactly that plan
    res, images = be.eng.segment_compact_groups(plan["groups"], plan["sources"], buf, plan["live"], conf["max_size"])
    for k, (files, lives) in enumerate(specs):
        want = ref_compact(files, lives, conf["max_size"])
        assert isinstance(want, bytes) and int(res["status"][k]) == OK and first_diff(images[k].tobytes(), want) is None, k


# ------------------------------------------------------------------------------------------ calling the batched copy

def pack_call(specs):
    """specs: [(files, lives)] per group -> (groups with their source slices, sources, files buffer, live pairs)"""
    files_all, lives_all = [], []
    groups = np.zeros(len(specs), dtype=abi.SEG_GROUP_DTYPE)
    for g, (files, lives) in enumerate(specs):
        groups[g] = (len(files_all), len(files), 0, 0)
        files_all += files
        lives_all += lives
    sources, buf, live = pack_group(files_all, lives_all)
    return groups, sources, buf, live


def lay_out(be, groups, sources, live, files_bytes, residues=None, short=()):
    """Guard bytes in front, between and behind the images: every group gets its bound (`short`: one byte less than
    the group's image needs is set by the caller) at an odd distance from its predecessor, or at the residue mod 16
    asked for.  -> (groups, bytes of out)"""
    laid, total, counts = be.engine.segment_compact_groups_bound(groups, sources, live, files_bytes)
    pos = 0
    for g in range(len(laid)):
        srcs = sources[int(laid["src_first"][g]):int(laid["src_first"][g]) + int(laid["src_n"][g])]
        assert int(laid["out_bytes"][g]) == 8 + 32 * int(counts[g]) + int(srcs["n_bytes"].sum())
        assert int(laid["out_offset"][g]) == pos, "the bound's own layout is back to back"
        pos += int(laid["out_bytes"][g])
    assert total == pos
    groups, pos = laid.copy(), GUARD
    for g in range(len(groups)):
        if residues is not None:
            pos += (residues[g] - pos) % 16
        else:
            pos += 1 + (5 * g) % 7
        groups["out_offset"][g] = pos
        pos += int(groups["out_bytes"][g])
    return groups, pos + GUARD, counts


def prepared_batch(be, groups, sources, buf, live, out_total, max_size=MAX_SIZE, flags=0, src_phase=0, dst_phase=0):
    """-> (call, fetch) as prepared_compact of tests/test_segment_compact.py: fetch() -> (result rows, all of out)"""
    n = len(groups)
    d_f, p_f, _ = be.dev(buf, src_phase)
    d_o, p_o, b_o = be.dev(np.full(out_total, 0xEE, dtype=np.uint8), dst_phase)
    d_r, p_r, b_r = be.dev(np.full(32 * n + 16, 0x77, dtype=np.uint8))

    def call():
        be.eng.segment_compact_groups_device(groups, sources, p_f, len(buf), live, p_o, out_total, p_r, max_size, flags)

    def fetch(_keep=d_f):
        got, rows = be.get(d_o), be.get(d_r)
        assert np.all(got[:b_o] == 0) and np.all(got[b_o + out_total:] == 0), "wrote outside the buffer"
        assert np.all(rows[b_r + 32 * n:b_r + 32 * n + 16] == 0x77), "wrote behind the result rows"
        return rows[b_r:b_r + 32 * n].copy().view(abi.SEG_COMPACT_RESULT_DTYPE), got[b_o:b_o + out_total].copy()
    return call, fetch


def run_batch(be, *args, **kw):
    call, fetch = prepared_batch(be, *args, **kw)
    call()
    return fetch()


def pad_call_to_width(specs, width):
    """Lengthen the last file of the call until (sum of the sources' n_bytes) / (live indexes of all groups) selects the
    lane-group width: 8 lanes up to 320, 16 below 1024, else a wavefront -- the rule of the batched call."""
    specs = [(list(f), l) for f, l in specs]
    n = max(1, sum(b - a + 1 for _, lives in specs for l in lives for a, b in l))
    total = sum(len(f) for files, _ in specs for f in files)
    want = {8: 0, 16: 600, 64: 1100}[width] * n
    last = max(g for g, (files, _) in enumerate(specs) if files)
    if total < want:
        specs[last][0][-1] = specs[last][0][-1] + b"\x3c" * (want - total)
    mean = sum(len(f) for files, _ in specs for f in files) // n
    assert {8: mean <= 320, 16: 320 < mean < 1024, 64: mean >= 1024}[width], (width, mean)
    return specs


def expected_row(want, out_bytes):
    """ref_compact's answer and the group's room -> (status, source, index) or None for a good image"""
    if isinstance(want, bytes):
        return (SPACE, 0, 0) if len(want) > out_bytes else None
    return want


def check_call(be, specs, max_size=MAX_SIZE, flags=0, width=None, residues=None, short=(), src_phase=0, dst_phase=0,
               host_form=True, share=None, what=""):
    """One batched call against both referees, group by group.  short: groups whose out_bytes is one byte less than
    their image.  share = (j, i): source j names the file bytes of source i.  -> (rows, out, groups, statuses)"""
    if width is not None:
        specs = pad_call_to_width(specs, width)
    groups, sources, buf, live = pack_call(specs)
    if share is not None:
        sources["offset"][share[0]] = sources["offset"][share[1]]
        assert int(sources["n_bytes"][share[0]]) == int(sources["n_bytes"][share[1]])
    groups, out_total, counts = lay_out(be, groups, sources, live, len(buf), residues)
    wants = [ref_compact(files, lives, max_size, bool(flags & VERIFY)) for files, lives in specs]
    for g in short:
        assert isinstance(wants[g], bytes)
        groups["out_bytes"][g] = len(wants[g]) - 1
    rows, out = run_batch(be, groups, sources, buf, live, out_total, max_size, flags, src_phase, dst_phase)
    owned = np.zeros(out_total, dtype=bool)
    statuses = []
    for g, (files, lives) in enumerate(specs):
        tag = f"{what} group {g}"
        off, room = int(groups["out_offset"][g]), int(groups["out_bytes"][g])
        first, n = int(groups["src_first"][g]), int(groups["src_n"][g])
        alone, region = device_compact(be, sources[first:first + n].copy(), buf, live, max_size, flags, out_bytes=room)
        for k in ROW_FIELDS:
            assert int(rows[k][g]) == int(alone[k]), f"{tag}: {k} {int(rows[k][g])}, alone {int(alone[k])}"
        want = expected_row(wants[g], room)
        if want is None:
            image = wants[g]
            assert (int(rows["status"][g]), int(rows["n_entries"][g]), int(rows["file_bytes"][g])) == \
                (OK, int(counts[g]), len(image)), f"{tag}: status {int(rows['status'][g])} index {int(rows['index'][g])}"
            diff = first_diff(out[off:off + len(image)].tobytes(), image)
            assert diff is None, f"{tag}: {diff}"
            assert first_diff(region[:len(image)].tobytes(), image) is None, f"{tag}: the call alone"
            owned[off:off + len(image)] = True
        else:
            got = (int(rows["status"][g]), int(rows["source"][g]), int(rows["index"][g]))
            assert got == want or (want[0] == SPACE and got[0] == SPACE), f"{tag}: {got} != {want}"
            if want[0] == SPACE:
                assert int(rows["file_bytes"][g]) == len(wants[g])
            owned[off:off + room] = True                    # its own output bytes are unspecified
        statuses.append(int(rows["status"][g]))
    assert np.all(out[~owned] == 0xEE), f"{what}: bytes outside the images were written"
    if host_form:
        host = np.full(out_total, 0xEE, dtype=np.uint8)
        res, images = be.eng.segment_compact_groups(groups, sources, buf, live, max_size, flags, out=host)
        good = np.zeros(out_total, dtype=bool)
        for g in range(len(specs)):
            for k in ROW_FIELDS:
                assert int(res[k][g]) == int(rows[k][g]), f"{what} group {g}, host-buffer form: {k}"
            if statuses[g] == OK:
                assert first_diff(images[g].tobytes(), wants[g]) is None, f"{what} group {g}, host-buffer form"
                good[int(groups["out_offset"][g]):int(groups["out_offset"][g]) + len(wants[g])] = True
            else:
                assert images[g] is None
        assert np.all(host[~good] == 0xEE), f"{what}: the host-buffer form wrote outside the good images"
    return rows, out, groups, statuses


# ------------------------------------------------------------------------------------------ building groups

def plain_group(rng, n_live, n_records=None, first=1, lens=None, hi=25, version=2, term=1):
    """One source of n_records records (default: n_live + 3) with small random payloads, n_live of them live -- every
    second record first, so that the live list has many pairs; `lens`: these payload lengths, every record live.
    -> (files, lives)"""
    n_records = n_live + 3 if n_records is None else n_records
    pay = rnd_payloads(rng, n_records, hi) if lens is None else \
        [rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes() for ln in lens]
    f = make_source([R(first + j, term, p) for j, p in enumerate(pay)], version=version)
    if lens is not None:
        return [f], [[(first, first + n_live - 1)]] if n_live else [[]]
    picked = [first + j for j in range(n_records)][::2][:n_live]
    picked += [first + j for j in range(1, n_records, 2)][:n_live - len(picked)]
    return [f], [ranges_of(picked)]


def boundary_specs(rng, width):
    """groups of 0, 1, PER_BLOCK - 1, PER_BLOCK and PER_BLOCK + 1 live entries next to each other, so that group edges
    fall in front of, on and behind workgroup edges of the copy, and a workgroup holds entries of up to four groups"""
    per = THREADS // width
    sizes = [per + 1, 0, 1, per - 1, per, 0, per + 1, 1, per, per - 1, per + 1]
    hi = {8: 60, 16: 200, 64: 300}[width]
    return [plain_group(rng, n, first=100 * g + 1, hi=hi) for g, n in enumerate(sizes)]


def mixed_specs(rng):
    """The kinds of group a member produces, in one call: trimmed and overwritten records, both file versions in one
    group, an index live in two sources, header-only groups first, in the middle and last, a source of more records
    than one step of the resolve pass, and two sources in different groups that share their file."""
    trimmed = source_of(rng, [1, 2, 3, 4, 5, 6, 7, 8, 4, 5, 9, 10, 10, 11])          # 6, 7, 8 trimmed; 10 overwritten
    assert sorted(ref_parse(trimmed)) == [1, 2, 3, 4, 5, 9, 10, 11]
    pay = rnd_payloads(rng, 30, 70)
    v1 = make_source([R(10 + j, 2, p) for j, p in enumerate(pay)], max_count=40, version=1)
    v2 = make_source([R(60 + j, 3, p) for j, p in enumerate(pay)])
    old = source_of(rng, list(range(1, 40)))
    new = make_source([R(i, 9, bytes([i]) * (i % 11)) for i in range(30, 60)])
    long = source_of(rng, list(range(500, 500 + CHUNK + 44)))
    shared = source_of(rng, list(range(700, 730)))
    empty = make_source([], max_count=16)
    return [([], []),                                                               # no sources: header only
            ([trimmed], [[(1, 5), (9, 11)]]),
            ([v1, v2], [[(10, 12), (20, 39)], [(61, 61), (70, 89)]]),
            ([empty, old], [[], []]),                                               # sources, nothing live: header only
            ([old, new], [[(1, 39)], [(30, 59)]]),
            ([shared], [[(700, 710)]]),
            ([long], [[(500, 500 + CHUNK + 43)]]),
            ([v2, shared], [[(60, 60)], [(715, 729)]]),
            ([], [])]


MIXED_SHARE = (10, 7)           # of mixed_specs: source 10 (group 7's second) names the file of source 7 (group 5's)


def check_boundaries(be, width):
    rng = np.random.default_rng(7400 + width)
    for flags in (0, VERIFY):
        _, _, _, st = check_call(be, boundary_specs(rng, width), flags=flags, width=width, what=f"width {width} flags {flags}")
        assert st == [OK] * 11


def check_mixed(be):
    rng = np.random.default_rng(7500)
    specs = mixed_specs(rng)
    for flags, dp in ((0, 0), (VERIFY, 11)):
        rows, _, _, st = check_call(be, specs, flags=flags, share=MIXED_SHARE, dst_phase=dp, src_phase=dp % 5, what=f"mixed, flags {flags}")
        assert st == [OK] * len(specs)
        assert [int(x) for x in rows["file_bytes"][[0, 3, 8]]] == [8, 8, 8] and int(rows["n_entries"][4]) == 39 + 30


def check_residues_and_lengths(be):
    """Image starts at every residue mod 16, the first and the last payload of an image 0, 1, 15, 16, 17 or 33 bytes"""
    rng = np.random.default_rng(7600)
    edge = [0, 1, 15, 16, 17, 33]
    specs = []
    for r in range(16):
        lens = [edge[r % 6]] + [int(x) for x in rng.integers(0, 40, size=r % 4)] + [edge[(r // 2 + 1) % 6]]
        specs.append(plain_group(rng, len(lens), first=50 * r + 1, lens=lens))
    for flags in (0, VERIFY):
        for dp in (0, 5):
            _, _, groups, st = check_call(be, specs, flags=flags, residues=[(r + 3) % 16 for r in range(16)], dst_phase=dp,
                                          host_form=dp == 0, what=f"residues, flags {flags} phase {dp}")
            assert st == [OK] * 16 and sorted(int(o) % 16 for o in groups["out_offset"]) == list(range(16))


def check_many_sources(be):
    """300 two-record sources in 150 groups: more sources than one rgb_segment_compact call takes"""
    rng = np.random.default_rng(7700)
    specs = []
    for g in range(150):
        a = make_source([R(10 * g + 1, 1, bytes([g % 251]) * (g % 19)), R(10 * g + 2, 1, b"xy")])
        b = make_source([R(10 * g + 3, 2, bytes([g % 7]) * 21), R(10 * g + 4, 2, b"")])
        specs.append(([a, b], [[(10 * g + 1 + g % 2, 10 * g + 2)], [(10 * g + 3, 10 * g + 3 + (g // 2) % 2)]]))
    assert sum(len(f) for f, _ in specs) == 300 > abi.SEG_COMPACT_MAX_SOURCES
    _, _, _, st = check_call(be, specs, flags=VERIFY, what="300 sources")
    assert st == [OK] * 150


def good_neighbours(rng):
    return plain_group(rng, 5, first=1, hi=12), plain_group(rng, 7, first=201, hi=12)


def status_cases(rng):
    """(name, the middle group, max_size, flags, short, the row expected)"""
    pay = [bytes([j]) * 100 for j in range(12)]
    s0 = make_source([R(1 + j, 1, p) for j, p in enumerate(pay[:6])])
    s1 = make_source([R(7 + j, 1, p) for j, p in enumerate(pay[6:])])
    trunc = [R(1 + j, 1, p) for j, p in enumerate(rnd_payloads(rng, 10, 80))]
    trunc[6]["ln"] = 5000
    bad_crc = [R(1 + j, 1, p) for j, p in enumerate(rnd_payloads(rng, 10, 80))]
    bad_crc[3]["payload"] += b"q" * 20
    bad_crc[3]["crc"] = 0x1234567
    return [("BAD_SOURCE", ([s0, b"RASX" + s1[4:]], [[(1, 6)], [(7, 12)]]), MAX_SIZE, 0, (), (BAD_SOURCE, 1, 0)),
            ("MISSING", ([s0, s1], [[(1, 6)], [(7, 13)]]), MAX_SIZE, 0, (), (MISSING, 1, 13)),
            ("TRUNCATED", ([s0, make_source(trunc)], [[(1, 6)], [(1, 10)]]), MAX_SIZE, 0, (), (TRUNCATED, 1, 7)),
            ("FULL", ([s0, s1], [[(1, 6)], [(7, 12)]]), 750, 0, (), (FULL, 1, 9)),
            ("SPACE", ([s0, s1], [[(1, 6)], [(7, 12)]]), MAX_SIZE, 0, (1,), (SPACE, 0, 0)),
            ("CRC", ([s0, make_source(bad_crc)], [[(1, 6)], [(2, 9)]]), MAX_SIZE, VERIFY, (), (CRC, 1, 4)),
            ("CRC without the flag", ([s0, make_source(bad_crc)], [[(1, 6)], [(2, 9)]]), MAX_SIZE, 0, (), None)]


def check_neighbours_untouched(be, specs, failing, max_size, flags, short, what):
    """The call with the failing groups, and the same call without their descriptors: every other group's row and image
    are bit-identical, and so is every byte outside the failing groups' ranges."""
    groups, sources, buf, live = pack_call(specs)
    groups, out_total, _ = lay_out(be, groups, sources, live, len(buf))
    for g in short:
        groups["out_bytes"][g] = len(ref_compact(*specs[g])) - 1
    rows, out = run_batch(be, groups, sources, buf, live, out_total, max_size, flags)
    keep = [g for g in range(len(specs)) if g not in failing]
    rows2, out2 = run_batch(be, groups[keep], sources, buf, live, out_total, max_size, flags)
    assert rows[keep].tobytes() == rows2.tobytes(), what
    mask = np.ones(out_total, dtype=bool)
    for g in failing:
        mask[int(groups["out_offset"][g]):int(groups["out_offset"][g]) + int(groups["out_bytes"][g])] = False
    assert np.array_equal(out[mask], out2[mask]), what


def check_statuses(be):
    rng = np.random.default_rng(7800)
    left, right = good_neighbours(rng)
    for name, middle, max_size, flags, short, want in status_cases(rng):
        specs = [left, middle, right]
        rows, _, _, st = check_call(be, specs, max_size=max_size, flags=flags, short=short, what=name)
        assert st[0] == OK and st[2] == OK, name
        if want is None:
            assert st[1] == OK, name
            continue
        assert st[1] == want[0] and (want[0] == SPACE or (int(rows["source"][1]), int(rows["index"][1])) == want[1:]), name
        check_neighbours_untouched(be, specs, [1], max_size, flags, short, name)
    # two failing groups with different statuses in one call, a good one between and around them
    cases = {c[0]: c for c in status_cases(rng)}
    specs = [left, cases["MISSING"][1], right, cases["TRUNCATED"][1], plain_group(rng, 3, first=900), cases["BAD_SOURCE"][1]]
    _, _, _, st = check_call(be, specs, what="three failing groups")
    assert st == [OK, MISSING, OK, TRUNCATED, OK, BAD_SOURCE]
    check_neighbours_untouched(be, specs, [1, 3, 5], MAX_SIZE, 0, (), "three failing groups")


def check_precedence(be, flags):
    """The precedence pairs of tests/test_segment_compact.py::check_status_precedence, in the second of three groups"""
    rng = np.random.default_rng(7900)
    left, right = good_neighbours(rng)
    clean, k = (20, None, None), 7
    for name, srcs, full, bad_crc, broken in (
            ("MISSING and TRUNCATED at one place", [(30, k, k)], None, None, None),
            ("MISSING and FULL at one place", [clean, (30, k, None)], (1, k), None, None),
            ("TRUNCATED and FULL at one place", [clean, (30, None, k)], (1, k), None, None),
            ("all three at one place", [clean, (30, k, k)], (1, k), None, None),
            ("TRUNCATED, MISSING one source later", [clean, (30, None, k), (10, 0, None)], None, None, None),
            ("FULL, MISSING at the last rank one source earlier", [(20, 19, None), (30, None, None)], (1, k), None, None),
            ("BAD_SOURCE behind all three", [(30, k, k), clean], (0, k), None, 1),
            ("BAD_SOURCE behind a Crc mismatch", [(30, None, None), clean], None, (0, 3), 1),
            ("MISSING behind a Crc mismatch", [(30, k, None)], None, (0, k - 1), None),
            ("the mismatch alone", [(30, None, None)], None, (0, k - 1), None)):
        files, lives, max_size, expect = precedence_group(srcs, full, bad_crc, broken)
        rows, _, _, st = check_call(be, [left, (files, lives), right], max_size=max_size, flags=flags, host_form=False, what=name)
        if expect is None:
            expect = (CRC, 0, k) if flags & VERIFY else None
        assert st[0] == OK and st[2] == OK, name
        got = None if st[1] == OK else (st[1], int(rows["source"][1]), int(rows["index"][1]))
        assert got == expect, f"{name}: {got}, the places say {expect}"


def check_verify(be):
    rng = np.random.default_rng(8000)

    def group(first, bad=(), zero=()):
        pay = rnd_payloads(rng, 12, 90)
        recs = [R(first + j, 1, p + b"." * 20) for j, p in enumerate(pay)]
        for j in zero:
            recs[j]["crc"] = 0
        f = bytearray(make_source(recs))
        parsed = ref_parse(bytes(f))
        for j in bad:
            f[parsed[first + j][1] + 3] ^= 0x10
        return [bytes(f)], [[(first, first + 11)]]
    rows, _, _, st = check_call(be, [group(1), group(101, bad=[4]), group(201)], flags=VERIFY, what="a mismatch in group 2 only")
    assert st == [OK, CRC, OK] and (int(rows["source"][1]), int(rows["index"][1])) == (0, 105)
    _, _, _, st = check_call(be, [group(1), group(101, bad=[4]), group(201)], flags=0, what="... not looked at without the flag")
    assert st == [OK, OK, OK]
    _, _, _, st = check_call(be, [group(1, bad=[2], zero=[2]), group(101, zero=[0, 11])], flags=VERIFY, what="a stored Crc of 0")
    assert st == [OK, OK]
    rows, _, _, st = check_call(be, [group(1), group(101, bad=[9, 3, 6])], flags=VERIFY, what="three mismatches in one group")
    assert st == [OK, CRC] and int(rows["index"][1]) == 104
    rows, _, _, st = check_call(be, [group(1, bad=[7]), group(101), group(201, bad=[1, 10]), group(301, bad=[11])], flags=VERIFY,
                                what="mismatches in three groups")
    assert st == [CRC, OK, CRC, CRC] and [int(x) for x in rows["index"][[0, 2, 3]]] == [8, 202, 312]


def check_argument_errors(be):
    rng = np.random.default_rng(8100)
    specs = [plain_group(rng, 4, first=1), plain_group(rng, 3, first=101)]
    groups, sources, buf, live = pack_call(specs)
    groups, out_total, _ = lay_out(be, groups, sources, live, len(buf))
    d_f, p_f, _ = be.dev(buf)
    d_o, p_o, b_o = be.dev(np.full(out_total + 64, 0xEE, dtype=np.uint8))

    def refused(name, grp=groups, srcs=sources, lv=live, files_bytes=len(buf), out_bytes=out_total, flags=0, p_out=p_o,
                p_res=p_o + out_total, bound=True):
        with pytest.raises(be.engine.RgbError) as e:
            be.eng.segment_compact_groups_device(grp, srcs, p_f, files_bytes, lv, p_out, out_bytes, p_res, MAX_SIZE, flags)
        assert e.value.code == E_INVAL, name
        host = np.full(out_bytes, 0xEE, dtype=np.uint8)
        if p_out and p_res:
            with pytest.raises(be.engine.RgbError) as e:
                be.eng.segment_compact_groups(grp, srcs, buf[:files_bytes], lv, MAX_SIZE, flags, out=host)
            assert e.value.code == E_INVAL and np.all(host == 0xEE), name
        if bound:
            with pytest.raises(be.engine.RgbError) as e:
                be.engine.segment_compact_groups_bound(grp, srcs, lv, files_bytes)
            assert e.value.code == E_INVAL, name

    def edit(arr, i, **kw):
        arr = arr.copy()
        for k, v in kw.items():
            arr[k][i] = v
        return arr
    refused("a group slice outside the sources", grp=edit(groups, 1, src_n=2))
    refused("a group slice that wraps", grp=edit(groups, 1, src_first=0xFFFFFFFF, src_n=2))
    refused("group slices that overlap", grp=edit(groups, 1, src_first=0))
    refused("overlapping out ranges", grp=edit(groups, 1, out_offset=int(groups["out_offset"][0]) + int(groups["out_bytes"][0]) - 1),
            bound=False)
    refused("the same out range twice", grp=edit(groups, 1, out_offset=int(groups["out_offset"][0])), bound=False)
    refused("an out range outside out_bytes", out_bytes=out_total - GUARD - 1, bound=False)
    refused("an out range that wraps", grp=edit(groups, 1, out_offset=(1 << 64) - 8), bound=False)
    refused("unknown flags", flags=2, bound=False)
    refused("a source outside the files buffer", files_bytes=len(buf) - 6)
    refused("a live slice outside the list", srcs=edit(sources, 1, live_n=40))
    refused("MaxCount 65536", lv=np.concatenate([live[:-1], np.array([[int(live[-1][0]), int(live[-1][0]) + 65535]], dtype=np.uint64)]))
    refused("live pairs not ascending", lv=live[::-1].copy() if len(live) > 1 else live)
    # live slices of two named sources that share a pair from different first pairs: the pair's rank cannot serve both
    assert len(live) >= 6
    refused("live slices that overlap in part", srcs=edit(edit(sources, 0, live_first=0, live_n=2), 1, live_first=1, live_n=2))
    refused("a live slice inside another", srcs=edit(edit(sources, 0, live_first=0, live_n=3), 1, live_first=2, live_n=1))
    refused("no out buffer", p_out=0, bound=False)
    refused("no result rows", p_res=0, bound=False)
    with pytest.raises(be.engine.RgbError) as e:
        be.eng._check(be.eng._L.rgb_segment_compact_groups_device(be.eng._h, None, 2, sources.ctypes.data, 2, p_f, len(buf),
                                                                  live.ctypes.data, len(live), MAX_SIZE, 0, p_o, out_total,
                                                                  p_o + out_total, None), "no groups")
    assert e.value.code == E_INVAL
    with pytest.raises(be.engine.RgbError) as e:
        be.eng._check(be.eng._L.rgb_segment_compact_groups_device(be.eng._h, groups.ctypes.data, 2, None, 2, p_f, len(buf),
                                                                  live.ctypes.data, len(live), MAX_SIZE, 0, p_o, out_total,
                                                                  p_o + out_total, None), "no sources")
    assert e.value.code == E_INVAL
    assert np.all(be.get(d_o)[b_o:b_o + out_total + 64] == 0xEE), "refused, but something was written"
    # slices that are the same from their first pair on are legal, whatever their lengths
    same = edit(edit(sources, 0, live_first=0, live_n=2), 1, live_first=0, live_n=1)
    same["offset"][1], same["n_bytes"][1] = same["offset"][0], same["n_bytes"][0]
    laid, _, counts = be.engine.segment_compact_groups_bound(groups, same, live, len(buf))
    assert [int(c) for c in counts] == [2, 1]
    # the limits themselves are legal: no groups at all, a group of 65535 live indexes (bound only), touching ranges
    be.eng.segment_compact_groups_device(groups[:0], sources, p_f, len(buf), live, 0, 0, 0)
    one = np.zeros(1, dtype=abi.SEG_SOURCE_DTYPE); one["n_bytes"], one["live_n"] = 100, 1
    g1 = np.zeros(1, dtype=abi.SEG_GROUP_DTYPE); g1["src_n"] = 1
    laid, total, counts = be.engine.segment_compact_groups_bound(g1, one, [(1, 65535)], 100)
    assert (total, int(counts[0]), int(laid["out_bytes"][0])) == (8 + 32 * 65535 + 100, 65535, 8 + 32 * 65535 + 100)
    assert np.all(be.get(d_o)[b_o:b_o + out_total + 64] == 0xEE)


def check_back_to_back_calls(be):
    """Two calls on a fresh context with nothing waited for in between: the first small, the second with more sources,
    groups, live pairs and plan entries, so that the pinned block, its device copy and the scratch plan are all regrown
    while the first call may still be under way (on the emulation each call runs to its end: the regrowth alone)."""
    rng = np.random.default_rng(8200)
    calls = [[plain_group(rng, 2, first=1)],
             [plain_group(rng, 40 + g, first=1000 * g + 1, hi=50) for g in range(12)] + [([], [])]]
    fresh = type(be)(be.engine)
    try:
        runs = []
        for specs in calls:
            groups, sources, buf, live = pack_call(specs)
            groups, out_total, _ = lay_out(fresh, groups, sources, live, len(buf))
            runs.append((specs, groups, prepared_batch(fresh, groups, sources, buf, live, out_total, flags=VERIFY)))
        for _, _, (call, _) in runs:
            call()
        for specs, groups, (_, fetch) in runs:
            rows, out = fetch()
            owned = np.zeros(len(out), dtype=bool)
            for g, (files, lives) in enumerate(specs):
                want = ref_compact(files, lives, verify=True)
                off = int(groups["out_offset"][g])
                assert int(rows["status"][g]) == OK and first_diff(out[off:off + len(want)].tobytes(), want) is None, g
                owned[off:off + len(want)] = True
            assert np.all(out[~owned] == 0xEE)
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------ CPU (emulation)

def test_abi_mirror():
    flat = " ".join(open(os.path.join(ROOT, "include", "ra_gpu_wal.h")).read().split())
    for name, val in (("RGB_SEG_PICK_UNREFERENCED", abi.SEG_PICK_UNREFERENCED), ("RGB_SEG_TAKE_OK", abi.SEG_TAKE_OK),
                      ("RGB_SEG_TAKE_BADARITH", abi.SEG_TAKE_BADARITH), ("RGB_SEG_GROUP_NONE", abi.SEG_GROUP_NONE)):
        assert int(flat.split(f"#define {name} ")[1].split()[0].rstrip("ul"), 0) == val, name
    assert abi.SEG_PICK_DTYPE.fields["live_first"][1] == 8 and abi.SEG_GROUP_DTYPE.fields["out_offset"][1] == 8
    assert abi.SEG_TAKE_MEMBER_DTYPE.fields["n_groups"][1] == 8 and abi.SEG_MEMBER_DTYPE.fields["live_first"][1] == 8


@pytest.mark.parametrize("width", [8, 16, 64])
def test_emu_group_boundaries(emu, width):
    check_boundaries(emu, width)


def test_emu_mixed(emu):
    check_mixed(emu)


def test_emu_residues_and_lengths(emu):
    check_residues_and_lengths(emu)


def test_emu_many_sources(emu):
    check_many_sources(emu)


def test_emu_statuses(emu):
    check_statuses(emu)


@pytest.mark.parametrize("flags", [0, VERIFY], ids=["plain", "verify"])
def test_emu_status_precedence(emu, flags):
    check_precedence(emu, flags)


def test_emu_verify(emu):
    check_verify(emu)


@pytest.mark.parametrize("sched", PERMUTED_SCHEDULES)
def test_emu_under_permuted_schedules(emu, sched):
    """Workgroups and lanes reversed and permuted (tests/emu_schedule.py): the per-group minimum of the Crc mismatches
    and the resolve pass's minima arrive in another order, the answers stay those of the referees."""
    with schedule(emu.engine, sched):
        check_mixed(emu)
        check_verify(emu)
        check_boundaries(emu, 16)


def test_emu_argument_errors(emu):
    check_argument_errors(emu)


def test_emu_back_to_back_calls(emu):
    check_back_to_back_calls(emu)


def test_emu_major_compaction_plan(emu):
    check_plan(emu)


def malformed_and_good_cases():
    """(kind, header values, arrays) for the harness: valid, boundary and malformed input of the three helpers"""
    U = (1 << 64) - 1
    M, TM, G, S = abi.SEG_MEMBER_DTYPE, abi.SEG_TAKE_MEMBER_DTYPE, abi.SEG_GROUP_DTYPE, abi.SEG_SOURCE_DTYPE

    def rows(dtype, *vals):
        a = np.zeros(len(vals), dtype=dtype)
        for i, v in enumerate(vals):
            a[i] = v
        return a

    def pairs(*p):
        return np.array(p, dtype=np.uint64).reshape(-1, 2)
    refs, live = pairs((300, 399), (200, 299), (100, 199)), pairs((150, 250), (290, 310))
    sel = [(rows(M, (0, 3, 0, 2)), refs, live, 5, 0), (rows(M, (0, 3, 0, 2)), refs, live, 4, 0),
           (rows(M, (0, 3, 0, 2)), refs, live, 3, 0), (rows(M, (0, 3, 0, 2)), refs, live, 0, 1),
           (rows(M, (0, 1, 0, 1), (1, 2, 1, 1)), refs, live, 8, 0), (rows(M), pairs(), pairs(), 0, 0),
           (rows(M, (0, 0, 0, 0)), pairs(), pairs(), 0, 0), (rows(M, (0, 1, 0, 1)), pairs((0, U)), pairs((0, U)), 1, 0),
           (rows(M, (0, 4, 0, 2)), refs, live, 8, 0), (rows(M, (0, 3, 2, 1)), refs, live, 8, 0),
           (rows(M, (0, 3, 0xFFFFFFFF, 2)), refs, live, 8, 0), (rows(M, (0, 3, 0, 2)), refs, pairs((5, 9), (10, 12)), 8, 0),
           (rows(M, (0, 2, 0, 2), (1, 2, 0, 2)), refs, live, 8, 0)]
    info = info_rows([I(100, 40)[0], I(100, 45)[0], I(0, 0)[0], I(4, 2, live_size=0, data=0)[0]])
    nl = np.array([40, 45, 0, 2], dtype=np.uint64)
    take = [(rows(TM, (0, 2, 0, 0)), info, nl, 128, 128_000), (rows(TM, (0, 2, 0, 0), (2, 1, 0, 0), (3, 1, 0, 0)), info, nl, 50, 9),
            (rows(TM, (0, 4, 0, 0)), info, nl, 128, 128_000), (rows(TM), info[:0], nl[:0], 1, 1),
            (rows(TM, (4, 0, 0, 0)), info, nl, 1, 1), (rows(TM, (1, 4, 0, 0)), info, nl, 1, 1),
            (rows(TM, (0, 2, 0, 0), (1, 2, 0, 0)), info, nl, 1, 1), (rows(TM, (0xFFFFFFFF, 2, 0, 0)), info, nl, 1, 1)]
    srcs = rows(S, (0, 40, 0, 2, 0), (40, 50, 2, 0, 0), (90, 10, 2, 1, 0))
    lv = pairs((1, 5), (7, 7), (3, 65000))
    bound = [(rows(G, (0, 2, 0, 0), (2, 1, 0, 0)), srcs, lv, 100), (rows(G, (0, 0, 0, 0), (0, 3, 0, 0), (3, 0, 0, 0)), srcs, lv, 100),
             (rows(G), srcs[:0], pairs(), 0), (rows(G, (0, 3, 0, 0)), srcs, pairs((1, 5), (7, 7), (3, 65530)), 100),
             (rows(G, (0, 4, 0, 0)), srcs, lv, 100), (rows(G, (2, 1, 0, 0), (0, 2, 0, 0)), srcs, lv, 100),
             (rows(G, (0, 3, 0, 0)), srcs, lv, 99), (rows(G, (0, 3, 0, 0)), srcs, pairs((1, 5), (6, 7), (9, 9)), 100),
             (rows(G, (0, 3, 0, 0)), srcs, lv[:2], 100), (rows(G, (0xFFFFFFFF, 2, 0, 0)), srcs, lv, 100),
             (rows(G, (0, 1, 0, 0), (1, 2, 0, 0)), rows(S, (0, 40, 0, 2, 0), (40, 50, 2, 0, 0), (90, 10, 1, 1, 0)), lv, 100)]
    return sel, take, bound


def test_plan_helpers_under_sanitizers(tmp_path, emulated_engine):
    """The three pure helpers -- rgb_segment_compact_select, _take_groups, _groups_bound, host-only code of
    rgb_segment_host.cpp -- compiled with AddressSanitizer + UBSan into a stand-alone program and run over valid,
    boundary and malformed input, every array in an exactly-sized heap block.  What the program prints is compared
    with what the library loaded into this process answers for the same input."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "segment_compact_groups_harness"
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-o", str(exe),
           os.path.join(ROOT, "tests", "native", "segment_compact_groups_harness.cpp"),
           os.path.join(ROOT, "ra_amd", "csrc", "rgb_segment_host.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert built.returncode == 0, built.stderr
    eng = emulated_engine
    sel, take, bound = malformed_and_good_cases()
    files, want = [], []

    def case(kind, a, b, c, x, y, *arrays):
        path = tmp_path / f"c{len(files)}.bin"
        path.write_bytes(struct.pack("<IIIIQQ", kind, a, b, c, x, y) + b"".join(arr.tobytes() for arr in arrays))
        files.append(str(path))
    for mem, refs, live, cap, sizing in sel:
        case(0, len(mem), len(refs), len(live), cap, sizing, mem, refs, live)
        try:
            if sizing:
                want.append([0, eng.segment_compact_select(mem, refs, live, sizing=True)])
                continue
            picks, out = eng.segment_compact_select(mem, refs, live)
            if len(out) > cap:
                raise eng.RgbError(E_INVAL, "cap")
            want.append([0, len(out)] + [int(p[k]) for p in picks for k in ("num_live", "live_first", "live_n", "flags")] +
                        [int(x) for x in out.reshape(-1)])
        except eng.RgbError as e:
            want.append([e.code, 0])
    for mem, info, nl, mc, ms in take:
        case(1, len(mem), len(info), 0, mc, ms, mem, info, nl)
        try:
            took, group_of = eng.segment_compact_take_groups(mem, info, nl, mc, ms)
            want.append([0] + [int(t[k]) for t in took for k in ("n_groups", "status")] + [int(g) for g in group_of])
        except eng.RgbError as e:
            want.append([e.code])
    for grp, srcs, lv, fb in bound:
        case(2, len(grp), len(srcs), len(lv), fb, 0, grp, srcs, lv)
        try:
            laid, total, counts = eng.segment_compact_groups_bound(grp, srcs, lv, fb)
            want.append([0, total] + [int(v) for g in range(len(laid))
                                      for v in (laid["out_offset"][g], laid["out_bytes"][g], counts[g])])
        except eng.RgbError as e:
            want.append([e.code, 0])
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    got = [[int(x) for x in line.split()] for line in run.stdout.splitlines()]
    assert got == want
    codes = [w[0] for w in want]
    assert codes[:len(sel)] == [0, 0, E_INVAL, 0, 0, 0, 0, 0] + [E_INVAL] * 5
    assert codes[len(sel):len(sel) + len(take)] == [0, 0, 0, 0, 0] + [E_INVAL] * 3
    assert codes[len(sel) + len(take):] == [0, 0, 0, 0] + [E_INVAL] * 7


def test_batched_compact_kernels_use_no_scratch():
    """hipcc's resource remarks for gfx950 (no GPU needed), as tests/test_segment_compact.py reads them: place, finish
    and the six copies of the batched call without scratch or spills; the copy without VERIFY holds no CRC tables."""
    from test_kernel_resources import segment_usage
    usage = segment_usage()
    names = [k for k in usage if "rgb_cgroups_" in k]
    assert len(names) == 8, names                       # place, finish, 3 widths x {verify, plain}
    for k in names:
        u = usage[k]
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, f"{k}: {u}"
        assert u["Occupancy"] >= 7 and u["LDS Size"] <= 20 * 1024 + 64, f"{k}: {u}"
        if "copy_kernel" in k and "ELb0E" in k:             # <GROUP, VERIFY = false>
            assert u["LDS Size"] <= 64, f"{k}: the plain copy must not hold the CRC tables"


# ------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("width", [8, 16, 64])
def test_gpu_group_boundaries(gpu, width):
    check_boundaries(gpu, width)


@pytest.mark.gpu
def test_gpu_mixed(gpu):
    check_mixed(gpu)


@pytest.mark.gpu
def test_gpu_residues_and_lengths(gpu):
    check_residues_and_lengths(gpu)


@pytest.mark.gpu
def test_gpu_many_sources(gpu):
    check_many_sources(gpu)


@pytest.mark.gpu
def test_gpu_statuses(gpu):
    check_statuses(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, VERIFY], ids=["plain", "verify"])
def test_gpu_status_precedence(gpu, flags):
    check_precedence(gpu, flags)


@pytest.mark.gpu
def test_gpu_verify(gpu):
    check_verify(gpu)


@pytest.mark.gpu
def test_gpu_argument_errors(gpu):
    check_argument_errors(gpu)


@pytest.mark.gpu
def test_gpu_back_to_back_calls(gpu):
    check_back_to_back_calls(gpu)


@pytest.mark.gpu
def test_gpu_major_compaction_plan(gpu):
    check_plan(gpu)
