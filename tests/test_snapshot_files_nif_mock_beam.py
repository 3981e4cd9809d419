"""crc32_spans/3, snapshot_build/3 and snapshot_validate/3 of the Erlang NIF shim (ra_amd/csrc/ra_gpu_batch_nif.c)
executed on the mock BEAM of tests/native/mock_beam, linked to the CPU-emulated library, under a Python twin of the
wrappers ra_gpu_batch:snapshot_images/2, snapshot_recover_batch/2 and accept_chunks/2 (erlang/ra_gpu_batch.erl, which no
OTP here can run): the twin builds the same binaries, calls the NIF and turns the answers into the same terms.
Answers against the referee of tests/test_snapshot_files.py (src/ra_log_snapshot.erl:49-108, 176-266)."""
import os
import re
import struct
import zlib

import numpy as np

from test_nif_shim_mock_beam import beam, ROOT          # noqa: F401  (the fixture that builds and loads the shim)
from test_snapshot_files import B, SNAPSHOT, ref_image, ref_info


# ---- the twin: erlang/ra_gpu_batch.erl, function by function

def snapshot_images(beam, ctx, snapshots):              # noqa: F811
    items, data, off, sizes = b"", b"", 0, []
    for meta, body in snapshots:
        items += struct.pack("<IIQQQQ", 0, len(meta), off, off + len(meta), len(body), 0)
        data += meta + body
        off += len(meta) + len(body)
        sizes.append(13 + len(meta) + len(body))
    got = beam.call("snapshot_build", ctx, items, data)
    if got[0] != "ok":
        return got
    images, out = got[1], []
    for size in sizes:
        out.append(images[:size]); images = images[size:]
    assert images == b""
    return ("ok", out)


def snapshot_recover_batch(beam, ctx, files):           # noqa: F811
    files_bin, blob, off = b"", b"", 0
    for file_bin, mode in files:
        files_bin += struct.pack("<QQIIQ", off, len(file_bin), 0, {"validate": 0, "read_meta": 1}[mode], 0)
        blob += file_bin
        off += len(file_bin)
    got = beam.call("snapshot_validate", ctx, files_bin, blob)
    if got[0] != "ok":
        return got
    out = []
    for st, v, _stored, _computed, m_off, m_len, _pad, d_off, d_len in struct.iter_unpack("<IIIIQIIQQ", got[1]):
        out.append({0: ("ok", blob[m_off:m_off + m_len], blob[d_off:d_off + d_len]), 1: ("error", "invalid_format"),
                    2: ("error", ("invalid_version", v)), 3: ("error", "checksum_error"), 4: ("error", "bad_meta"),
                    5: ("error", "unexpected_eof_when_parsing_header")}[st])
    return ("ok", out)


def accept_chunks(beam, ctx, chunks):                   # noqa: F811
    spans, data, off = b"", b"", 0
    for crc0, chunk in chunks:
        spans += struct.pack("<QQIIQ", off, len(chunk), crc0, 0, 0)
        data += chunk
        off += len(chunk)
    ok, crcs = beam.call("crc32_spans", ctx, spans, data)
    assert ok == "ok"
    return [c for (c,) in struct.iter_unpack("<I", crcs)]


def reference_answer(file_bin, mode):
    """recover/1 and read_meta_internal/1 in the wrapper's terms, from the referee's row"""
    st, v, _s, _c, m_off, m_len, d_off, d_len = ref_info(file_bin, 0, len(file_bin), SNAPSHOT, mode == "read_meta")
    return {0: ("ok", file_bin[m_off:m_off + m_len], file_bin[d_off:d_off + d_len]), 1: ("error", "invalid_format"),
            2: ("error", ("invalid_version", v)), 3: ("error", "checksum_error"), 4: ("error", "bad_meta"),
            5: ("error", "unexpected_eof_when_parsing_header")}[st]


# ---- the tests

def test_snapshot_nifs_and_the_wrappers_twin(beam):     # noqa: F811
    ok, ctx = beam.call("open", 0, 16, 2, 256)
    assert ok == "ok"
    rng = np.random.default_rng(46)

    # writing: many members' snapshots in one call
    snapshots = [(rng.bytes(int(rng.integers(0, 200))), rng.bytes(int(rng.integers(0, 3000)))) for _ in range(40)]
    snapshots += [(b"", b""), (rng.bytes(70), rng.bytes(B + 5)), (rng.bytes(17000), b"x")]
    got = snapshot_images(beam, ctx, snapshots)
    assert got == ("ok", [ref_image(SNAPSHOT, m, d) for m, d in snapshots])
    assert snapshot_images(beam, ctx, []) == ("ok", [])
    images = got[1]

    # a mixed recovery batch: snapshot (validate), newest checkpoint (validate), older checkpoints (read_meta), with
    # damaged, truncated, foreign and empty files among them
    hurt = bytearray(images[5]); hurt[-1] ^= 2
    old = bytearray(images[6]); old[4] = 0
    cut = images[7][:len(images[7]) - 3]
    lying = struct.pack(">4sBI", b"RASN", 1, zlib.crc32(struct.pack(">I", 50) + b"short")) + struct.pack(">I", 50) + b"short"
    batch = []
    for k, img in enumerate(images[:12] + [bytes(hurt), bytes(old), cut, lying, b"", b"RASN", images[3][:9], images[3][:11],
                                           struct.pack(">4sBI", b"RASN", 1, 0), b"RASI" + images[2][4:], images[41]]):
        batch += [(img, "validate"), (img, "read_meta")] if k % 3 != 1 else [(img, "read_meta"), (img, "validate")]
    got = snapshot_recover_batch(beam, ctx, batch)
    assert got == ("ok", [reference_answer(f, mode) for f, mode in batch])
    kinds = {a if a[0] == "error" else a[0] for a in got[1]}
    assert {"ok", ("error", "invalid_format"), ("error", ("invalid_version", 0)), ("error", ("invalid_version", 1)),
            ("error", "checksum_error"), ("error", "bad_meta"), ("error", "unexpected_eof_when_parsing_header")} <= kinds
    assert got[1][0] == ("ok", snapshots[0][0], snapshots[0][1])
    assert snapshot_recover_batch(beam, ctx, []) == ("ok", [])

    # receiving: chunk chains of several transfers in flight, a tick at a time
    transfers = [rng.bytes(n) for n in (0, 1, 700, 5000, B + 900, 20000)]
    cuts = [sorted(set([0, len(t)] + [int(x) for x in rng.integers(0, len(t) + 1, size=4)])) for t in transfers]
    crcs = [0] * len(transfers)
    for tick in range(5):
        live = [k for k in range(len(transfers)) if tick + 1 < len(cuts[k])]
        got = accept_chunks(beam, ctx, [(crcs[k], transfers[k][cuts[k][tick]:cuts[k][tick + 1]]) for k in live])
        for k, crc in zip(live, got):
            crcs[k] = crc
    assert crcs == [zlib.crc32(t) for t in transfers]
    assert accept_chunks(beam, ctx, []) == []

    # binaries of the wrong size, arguments of the wrong kind; malformed contents are the library's {error, invalid}
    span = struct.pack("<QQIIQ", 0, 4, 0, 0, 0)
    assert beam.call("crc32_spans", ctx, span, b"abcd") == ("ok", struct.pack("<I", zlib.crc32(b"abcd")))
    assert beam.call("crc32_spans", ctx, span[:-1], b"abcd") == "badarg"
    assert beam.call("crc32_spans", ctx, span, 7) == "badarg"
    assert beam.call("crc32_spans", ctx, span, b"abc") == ("error", "invalid")
    item = struct.pack("<IIQQQQ", 0, 2, 0, 2, 3, 0)
    assert beam.call("snapshot_build", ctx, item, b"mmddd") == ("ok", ref_image(SNAPSHOT, b"mm", b"ddd"))
    assert beam.call("snapshot_build", ctx, item + b"\0", b"mmddd") == "badarg"
    assert beam.call("snapshot_build", ctx, 5, b"mmddd") == "badarg"
    assert beam.call("snapshot_build", ctx, item, b"mmdd") == ("error", "invalid")
    assert beam.call("snapshot_build", ctx, struct.pack("<IIQQQQ", 2, 2, 0, 2, 3, 0), b"mmddd") == ("error", "invalid")
    assert beam.call("snapshot_build", ctx, struct.pack("<IIQQQQ", 1, 2, 0, 2, 3, 0), b"mmddd") == ("error", "invalid")
    assert beam.call("snapshot_build", ctx, struct.pack("<IIQQQQ", 0, 2, 0, 2, 1 << 62, 0), b"mmddd") == ("error", "invalid")
    one = struct.pack("<QQIIQ", 0, 9, 0, 0, 0)
    assert beam.call("snapshot_validate", ctx, one, images[3][:9])[0] == "ok"
    assert beam.call("snapshot_validate", ctx, one[:-2], images[3][:9]) == "badarg"
    assert beam.call("snapshot_validate", ctx, one, "atom") == "badarg"
    assert beam.call("snapshot_validate", ctx, one, images[3][:8]) == ("error", "invalid")
    assert beam.call("snapshot_validate", ctx, struct.pack("<QQIIQ", 0, 9, 0, 2, 0), images[3][:9]) == ("error", "invalid")
    assert beam.call("snapshot_validate", ctx, struct.pack("<QQIIQ", 0, 9, 3, 0, 0), images[3][:9]) == ("error", "invalid")
    beam.L.mock_gc_resource_term(ctx.t)


def test_snapshot_nifs_are_dirty_and_match_the_erlang_stubs(beam):                  # noqa: F811
    src = open(os.path.join(ROOT, "erlang", "ra_gpu_batch.erl")).read()
    stubs = dict(re.findall(r"^(\w+)\(([^)]*)\)\s*->\s*erlang:nif_error\(not_loaded\)\.", src, flags=re.M))
    for name in ("crc32_spans", "snapshot_build", "snapshot_validate"):
        assert len([x for x in stubs[name].split(",") if x.strip()]) == 3
        assert beam.L.mock_func_flags(name.encode(), 3) == 2, f"{name}: dirty IO-bound, as segment_read"
    assert "crc32_spans/3, snapshot_build/3, snapshot_validate/3, snapshot_images/2, snapshot_recover_batch/2, " \
           "accept_chunks/2" in src                                                 # exported
    assert "NOT COMPILED OR RUN" in src
