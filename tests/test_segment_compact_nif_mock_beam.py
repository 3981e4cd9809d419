"""segment_info/4 and segment_compact/6 of the Erlang NIF shim (ra_amd/csrc/ra_gpu_batch_nif.c) executed on the mock
BEAM of tests/native/mock_beam, linked to the CPU-emulated library: results against the referee of
tests/test_segment_compact.py (src/ra_log_segment.erl:736-790, 819-908, 1057-1116)."""
import os
import re

import numpy as np

from ra_amd import abi
from test_nif_shim_mock_beam import beam, ROOT          # noqa: F401  (the fixture that builds and loads the shim)
from test_segment_compact import R, make_source, pack_group, ranges_of, ref_compact, ref_info, ref_parse, source_of


def test_segment_compact_nifs(beam):                    # noqa: F811
    ok, ctx = beam.call("open", 0, 16, 2, 256)
    assert ok == "ok"
    rng = np.random.default_rng(16)
    a = source_of(rng, [1, 2, 3, 4, 5, 6, 3, 4, 7, 8, 9])
    b = make_source([R(8 + j, 5, bytes([j]) * (40 * j)) for j in range(12)], max_count=20, version=1)
    files = [a, b]
    lives = [ranges_of(k for k in ref_parse(a) if k != 5), [(8, 12), (15, 19)]]
    sources, buf, live = pack_group(files, lives)
    args = (sources.tobytes(), buf.tobytes(), live.tobytes())

    for live_bin, live_of in ((args[2], lambda s: lives[s]), (b"", lambda s: None)):
        ok, infos = beam.call("segment_info", ctx, args[0], args[1], live_bin)
        assert ok == "ok"
        rows = np.frombuffer(infos, dtype=abi.SEG_INFO_DTYPE)
        assert len(rows) == 2
        for s, f in enumerate(files):
            want = ref_info(f, live_of(s))
            for k in ("num_entries", "size", "index_size", "live_size", "max_count", "version"):
                assert int(rows[k][s]) == want[k], (s, k)
            assert int(rows["num_indexes"][s]) == len(want["indexes"])
            assert (int(rows["range_first"][s]), int(rows["range_last"][s])) == want["range"]

    want = ref_compact(files, lives)
    assert isinstance(want, bytes)
    for flags in (0, abi.SEG_COMPACT_VERIFY):
        assert beam.call("segment_compact", ctx, *args, abi.SEG_MAX_SIZE_B, flags) == ("ok", want)

    # what copy/3 and append_raw/6 fail with
    _, _, missing = pack_group(files, [[(1, 5)], [(8, 12)]])               # 5 and 6 went with the backwards step
    assert ref_compact(files, [[(1, 5)], [(8, 12)]])[0] == abi.SEG_COMPACT_MISSING
    src2 = sources.copy(); src2["live_n"] = (1, 1); src2["live_first"] = (0, 1)
    assert beam.call("segment_compact", ctx, src2.tobytes(), args[1], missing.tobytes(), abi.SEG_MAX_SIZE_B, 0) == \
        ("error", ("copy_missing_key", 5))
    assert ref_compact(files, lives, max_size=100)[0] == abi.SEG_COMPACT_FULL
    assert beam.call("segment_compact", ctx, *args, 100, 0) == ("error", "full")
    damaged = bytearray(buf.tobytes())
    off = int(sources["offset"][1]) + ref_parse(b)[10][1]
    damaged[off] ^= 1
    assert beam.call("segment_compact", ctx, args[0], bytes(damaged), args[2], abi.SEG_MAX_SIZE_B, 1) == \
        ("error", ("crc", 1, 10))
    assert ref_compact([a, bytes(damaged)[int(sources["offset"][1]):][:len(b)]], lives, verify=True) == \
        (abi.SEG_COMPACT_CRC, 1, 10)

    # binaries of the wrong size, arguments of the wrong kind; malformed contents are the library's {error, invalid}
    assert beam.call("segment_info", ctx, args[0][:-1], args[1], args[2]) == "badarg"
    assert beam.call("segment_info", ctx, args[0], args[1], args[2][:-8]) == "badarg"
    assert beam.call("segment_compact", ctx, args[0][:-1], args[1], args[2], abi.SEG_MAX_SIZE_B, 0) == "badarg"
    assert beam.call("segment_compact", ctx, args[0], args[1], args[2] + b"\0", abi.SEG_MAX_SIZE_B, 0) == "badarg"
    assert beam.call("segment_compact", ctx, args[0], args[1], args[2], abi.SEG_MAX_SIZE_B, 1 << 32) == "badarg"
    assert beam.call("segment_compact", ctx, args[0], args[1], args[2], abi.SEG_MAX_SIZE_B, 2) == ("error", "invalid")
    assert beam.call("segment_compact", ctx, args[0], args[1][:-200], args[2], abi.SEG_MAX_SIZE_B, 0) == ("error", "invalid")
    bad = bytearray(args[1]); bad[int(sources["offset"][0])] = ord("X")
    assert beam.call("segment_info", ctx, args[0], bytes(bad), args[2]) == ("error", "invalid")
    beam.L.mock_gc_resource_term(ctx.t)


def test_segment_compact_nifs_are_dirty_and_match_the_erlang_stub(beam):            # noqa: F811
    src = open(os.path.join(ROOT, "erlang", "ra_gpu_batch.erl")).read()
    stubs = dict(re.findall(r"^(\w+)\(([^)]*)\)\s*->\s*erlang:nif_error\(not_loaded\)\.", src, flags=re.M))
    for name, arity in (("segment_info", 4), ("segment_compact", 6)):
        assert len([a for a in stubs[name].split(",") if a.strip()]) == arity
        assert beam.L.mock_func_flags(name.encode(), arity) == 2, f"{name}: dirty IO-bound, as wal_frame"
    assert "segment_info/4, segment_compact/6, segment_compact_group/4" in src      # exported
    assert "NOT COMPILED OR RUN" in src
