"""wal_batch/6 of the Erlang NIF shim (ra_amd/csrc/ra_gpu_batch_nif.c) executed on the mock BEAM of
tests/native/mock_beam, linked to the CPU-emulated library: binaries in, {ok, {ResultsBin, WritersBin}, FramedBin,
{EventsBin, RangesBin}, TotalBin} out, over the cases of tests/golden/ra_log_wal_suite_batches.json and compared with
the referee of tests/test_wal_batch.py.  wal_handle_batch/5 of erlang/ra_gpu_batch.erl is restated here over the NIF's
binaries (no Erlang/OTP in this environment): the answer it would build is what the suite states."""
import os
import re

import numpy as np
import pytest

from ra_amd import abi
from test_nif_shim_mock_beam import beam, ROOT          # noqa: F401  (the fixture that builds and loads the shim)
from test_wal_batch import (GOLDEN_NAMES, ROLL, VERDICT_NAMES, check_against, golden_cases, golden_inputs, pack, referee,
                            small_case)


def handle_batch(beam, ctx, ca, wa, fa, data, flags=0):         # noqa: F811
    """wal_handle_batch/5's decoding of the NIF's answer -> (verdicts, framed, writers, events, file, roll)"""
    ok, (results_bin, writers_bin), framed, (events_bin, ranges_bin), total_bin = \
        beam.call("wal_batch", ctx, ca.tobytes(), wa.tobytes(), fa.tobytes(), data.tobytes(), flags)
    assert ok == "ok" and len(results_bin) == 16 * len(ca) and len(writers_bin) == 32 * len(wa) and len(total_bin) == 64
    total = np.frombuffer(total_bin, dtype=abi.WAL_BATCH_TOTAL_DTYPE)[0]
    results = np.frombuffer(results_bin, dtype=abi.WAL_CMD_RESULT_DTYPE)
    writers = np.frombuffer(writers_bin, dtype=abi.WAL_WRITER_DTYPE)
    events = np.frombuffer(events_bin, dtype=abi.WAL_EVENT_DTYPE)
    ranges = np.frombuffer(ranges_bin, dtype=np.uint64).reshape(-1, 2)
    assert (len(framed), len(events), len(ranges)) == (int(total["out_bytes"]), int(total["n_events"]), int(total["n_ranges"]))
    return total, results, writers, np.frombuffer(framed, dtype=np.uint8), events, ranges


@pytest.mark.parametrize("case_name", GOLDEN_NAMES)
def test_wal_batch_nif_over_the_suite_cases(beam, case_name):                 # noqa: F811
    ok, ctx = beam.call("open", 0, 16, 2, 256)
    assert ok == "ok"
    uid, cases = golden_cases()
    case = next(c for c in cases if c["name"] == case_name)
    cmds, writers = golden_inputs(uid, case)
    ca, wa, fa, data = pack(np.random.default_rng(8), cmds, writers, next_id_ref=1, max_size=case["max_size"],
                            max_entries=case["max_entries"])
    got = handle_batch(beam, ctx, ca, wa, fa, data)
    ref = referee(cmds, writers, 0, 0, 1, case["max_size"], case["max_entries"])
    check_against(ref, got, 1)
    total, results = got[0], got[1]
    assert [int(v) & abi.WAL_V_MASK for v in results["verdict"]] == [VERDICT_NAMES[v] for v in case["verdicts"]]
    roll = ("roll", int(total["n_consumed"])) if int(total["status"]) == ROLL else "ok"
    assert roll == (("roll", case["n_consumed"]) if case["status"] == "roll" else "ok")
    beam.L.mock_gc_resource_term(ctx.t)


def test_wal_batch_nif_arguments(beam):                                       # noqa: F811
    ok, ctx = beam.call("open", 0, 16, 2, 256)
    assert ok == "ok"
    cmds, writers = small_case()
    ca, wa, fa, data = pack(np.random.default_rng(9), cmds, writers, next_id_ref=3)
    got = handle_batch(beam, ctx, ca, wa, fa, data, abi.WAL_NO_CHECKSUMS)
    check_against(referee(cmds, writers, 0, 0, 3, 1 << 40, 0, checksums=False), got, len(writers), checksums=False)
    args = (ca.tobytes(), wa.tobytes(), fa.tobytes(), data.tobytes())
    empty = beam.call("wal_batch", ctx, b"", b"", args[2], b"", 0)
    assert empty[:4] == ("ok", (b"", b""), b"", (b"", b""))
    # binaries of the wrong size, arguments of the wrong kind; malformed contents are the library's {error, invalid}
    assert beam.call("wal_batch", ctx, args[0][:-1], args[1], args[2], args[3], 0) == "badarg"
    assert beam.call("wal_batch", ctx, args[0], args[1] + b"\0", args[2], args[3], 0) == "badarg"
    assert beam.call("wal_batch", ctx, args[0], args[1], args[2][:-8], args[3], 0) == "badarg"
    assert beam.call("wal_batch", ctx, args[0], args[1], args[2], 7, 0) == "badarg"
    assert beam.call("wal_batch", ctx, args[0], args[1], args[2], args[3], -1) == "badarg"
    assert beam.call("wal_batch", ctx, args[0], args[1], args[2], args[3], 2) == ("error", "invalid")
    assert beam.call("wal_batch", ctx, args[0], args[1][:-32], args[2], args[3], 0) == ("error", "invalid")   # a slot outside
    assert beam.call("wal_batch", ctx, args[0], args[1], args[2], args[3][:-40], 0) == ("error", "invalid")   # a payload outside
    beam.L.mock_gc_resource_term(ctx.t)


def test_wal_batch_nif_is_dirty_and_matches_the_erlang_stub(beam):            # noqa: F811
    src = open(os.path.join(ROOT, "erlang", "ra_gpu_batch.erl")).read()
    stubs = dict(re.findall(r"^(\w+)\(([^)]*)\)\s*->\s*erlang:nif_error\(not_loaded\)\.", src, flags=re.M))
    assert len([a for a in stubs["wal_batch"].split(",") if a.strip()]) == 6
    assert beam.L.mock_func_flags(b"wal_batch", 6) == 2, "wal_batch: dirty IO-bound, as wal_frame"
    assert "wal_batch/6, wal_handle_batch/5" in src                           # exported
    assert "NOT COMPILED OR RUN" in src
