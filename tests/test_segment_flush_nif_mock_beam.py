"""segment_flush/7 of the Erlang NIF shim (ra_amd/csrc/ra_gpu_batch_nif.c) executed on the mock BEAM of
tests/native/mock_beam, linked to the CPU-emulated library: binaries in, {ok, PiecesBin, OutBin} out, applied and
compared with the referee of tests/test_segment_flush.py (src/ra_log_segment.erl:252-338, 1250-1255;
src/ra_log_segment_writer.erl:425-500)."""
import os
import re

import numpy as np

from ra_amd import abi
from test_nif_shim_mock_beam import beam, ROOT          # noqa: F401  (the fixture that builds and loads the shim)
from test_segment_flush import build_call, check_answer, mk_writer


def test_segment_flush_nif(beam):                       # noqa: F811
    ok, ctx = beam.call("open", 0, 16, 2, 256)
    assert ok == "ok"
    rng = np.random.default_rng(26)
    specs = [mk_writer(rng, [int(x) for x in rng.integers(0, 60, size=n)], omax=5, ocount=w % 4, oidx=40 * w + 3)
             for w, n in enumerate((6, 0, 1, 19, 70))]
    specs[3]["entries"][5] = (2, 8, b"an index below the open range")
    writers, entries, data, batches = build_call(rng, specs, gaps=True)
    args = (writers.tobytes(), entries.tobytes(), data.tobytes())

    for max_count, max_size, flags in ((4, 100, 0), (3, 1 << 40, abi.SEG_NO_CHECKSUMS), (65535, 0, 0)):
        ok, pieces_bin, out = beam.call("segment_flush", ctx, *args, max_count, max_size, flags)
        assert ok == "ok" and len(pieces_bin) % 80 == 0
        pieces = np.frombuffer(pieces_bin, dtype=abi.SEG_PIECE_DTYPE)
        res = np.zeros(1, dtype=abi.SEG_FLUSH_RESULT_DTYPE)[0]
        res["n_pieces"], res["out_bytes"] = len(pieces), len(out)             # the binaries are cut to the answer
        want = check_answer(specs, batches, max_count, max_size, flags, res, pieces, out, f"max_count {max_count}")
        assert max(len(f) for f in want) >= 3
    assert beam.call("segment_flush", ctx, b"", b"", b"", 4, 100, 0) == ("ok", b"", b"")

    # binaries of the wrong size, arguments of the wrong kind; malformed contents are the library's {error, invalid}
    assert beam.call("segment_flush", ctx, args[0][:-1], args[1], args[2], 4, 100, 0) == "badarg"
    assert beam.call("segment_flush", ctx, args[0], args[1] + b"\0", args[2], 4, 100, 0) == "badarg"
    assert beam.call("segment_flush", ctx, args[0], args[1], args[2], 1 << 32, 100, 0) == "badarg"
    assert beam.call("segment_flush", ctx, args[0], args[1], args[2], 4, -1, 0) == "badarg"
    assert beam.call("segment_flush", ctx, args[0], args[1], 7, 4, 100, 0) == "badarg"
    assert beam.call("segment_flush", ctx, args[0], args[1], args[2], 4, 100, 2) == ("error", "invalid")
    assert beam.call("segment_flush", ctx, args[0], args[1], args[2], 0, 100, 0) == ("error", "invalid")
    assert beam.call("segment_flush", ctx, args[0], args[1], args[2], 65536, 100, 0) == ("error", "invalid")
    assert beam.call("segment_flush", ctx, args[0], args[1][:-64], args[2], 4, 100, 0) == ("error", "invalid")   # a slice outside
    assert beam.call("segment_flush", ctx, args[0], args[1], args[2][:-400], 4, 100, 0) == ("error", "invalid")  # a payload outside
    bad = writers.copy(); bad["open_count"][0] = 6                             # > open_max_count
    assert beam.call("segment_flush", ctx, bad.tobytes(), args[1], args[2], 4, 100, 0) == ("error", "invalid")
    beam.L.mock_gc_resource_term(ctx.t)


def test_segment_flush_nif_is_dirty_and_matches_the_erlang_stub(beam):              # noqa: F811
    src = open(os.path.join(ROOT, "erlang", "ra_gpu_batch.erl")).read()
    stubs = dict(re.findall(r"^(\w+)\(([^)]*)\)\s*->\s*erlang:nif_error\(not_loaded\)\.", src, flags=re.M))
    assert len([a for a in stubs["segment_flush"].split(",") if a.strip()]) == 7
    assert beam.L.mock_func_flags(b"segment_flush", 7) == 2, "segment_flush: dirty IO-bound, as wal_frame"
    assert "segment_flush/7, segment_flush_batch/5" in src                          # exported
    assert "NOT COMPILED OR RUN" in src
