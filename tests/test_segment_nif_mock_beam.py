"""crc32s/3, crc32_stream/3 and segment_build/5 of the Erlang NIF shim (ra_amd/csrc/ra_gpu_batch_nif.c) executed on
the mock BEAM of tests/native/mock_beam, linked to the CPU-emulated library: results against zlib.crc32 and the
struct.pack image of tests/test_segment.py (format: src/ra_log_segment.erl:41-45, 1118-1122, 1211-1219)."""
import os
import re
import zlib

import numpy as np

from ra_amd import abi
from test_nif_shim_mock_beam import beam, ROOT          # noqa: F401  (the fixture that builds and loads the shim)
from test_segment import pack_entries, python_segment


def test_segment_nifs(beam):                            # noqa: F811
    ok, ctx = beam.call("open", 0, 16, 2, 256)
    assert ok == "ok"
    rng = np.random.default_rng(15)
    lens = [0, 1, 15, 16, 17, 300, 1000, 5000] + [int(x) for x in rng.integers(0, 900, size=30)]
    entries, data, payloads = pack_entries(rng, lens)
    ok, crcs = beam.call("crc32s", ctx, entries.tobytes(), data.tobytes())
    assert ok == "ok"
    assert np.frombuffer(crcs, dtype="<u4").tolist() == [zlib.crc32(p) for p in payloads]
    assert beam.call("crc32s", ctx, entries.tobytes()[:-1], data.tobytes()) == "badarg"
    bad = entries.copy(); bad["data_len"][3] = len(data) + 1
    assert beam.call("crc32s", ctx, bad.tobytes(), data.tobytes())[0] == "error"

    blob = rng.integers(0, 256, size=200001, dtype=np.uint8).tobytes()
    assert beam.call("crc32_stream", ctx, blob, 0) == ("ok", zlib.crc32(blob))
    ok, part = beam.call("crc32_stream", ctx, blob[:77777], 0)                 # accept_chunk/2's chaining
    assert beam.call("crc32_stream", ctx, blob[77777:], part) == ("ok", zlib.crc32(blob))
    assert beam.call("crc32_stream", ctx, b"", 0x1234) == ("ok", 0x1234)
    assert beam.call("crc32_stream", ctx, blob, 1 << 32) == "badarg"

    keys = [(int(e["index"]), int(e["term"])) for e in entries]
    for max_count, flags in ((len(lens), 0), (4096, 0), (64, abi.SEG_NO_CHECKSUMS)):
        ok, image = beam.call("segment_build", ctx, entries.tobytes(), data.tobytes(), max_count, flags)
        assert ok == "ok" and image == python_segment(keys, payloads, max_count, not flags)
    assert beam.call("segment_build", ctx, entries.tobytes(), data.tobytes(), len(lens) - 1, 0)[0] == "error"
    assert beam.call("segment_build", ctx, entries.tobytes(), data.tobytes(), 65536, 0)[0] == "error"
    assert beam.call("segment_build", ctx, bad.tobytes(), data.tobytes(), 64, 0)[0] == "error"
    assert beam.call("segment_build", ctx, entries.tobytes()[:-5], data.tobytes(), 64, 0) == "badarg"
    beam.L.mock_gc_resource_term(ctx.t)


def test_segment_nifs_are_dirty_and_match_the_erlang_stub(beam):            # noqa: F811
    src = open(os.path.join(ROOT, "erlang", "ra_gpu_batch.erl")).read()
    stubs = dict(re.findall(r"^(\w+)\(([^)]*)\)\s*->\s*erlang:nif_error\(not_loaded\)\.", src, flags=re.M))
    for name, arity in (("crc32s", 3), ("crc32_stream", 3), ("segment_build", 5)):
        assert len([a for a in stubs[name].split(",") if a.strip()]) == arity
        assert beam.L.mock_func_flags(name.encode(), arity) == 2, f"{name}: dirty IO-bound, as wal_frame"
