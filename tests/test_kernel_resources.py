"""Register budget of the hot kernels (no GPU needed: hipcc's kernel-resource-usage remarks for gfx950, EVERY group size).

Round 5 found out the hard way that this is a CORRECTNESS gate, not a performance note: an opt-in code path added
inside handle_leader pushed rgb_tick_classes_kernel<5> over its 128-register budget (66 VGPRs spilled to scratch), and
on the MI355X that build returned wrong decisions for ~100 of 285 000 messages per tick -- always lanes 0-15 of a
wavefront, always in the general append_entries_rpc path, a different set on every run -- while the CPU emulation of
the same sources stayed bit-exact (tools/parity_tick0.py, profiles/EXPERIMENTS.md "Round 5").  That source was fixed
before it was committed and cannot be rebuilt; round 6 could not make the miscompare happen again on purpose (the class
kernel forced down to 96 registers -- 1 501 spill instructions, 196 bytes of scratch per lane -- is bit-exact over
full-size ticks on the device: profiles/r06_probes_counters_calibration.txt, and stays in the GPU suite:
tests/test_gpu_parity.py::test_forced_spill_class_kernel_is_bit_exact).  Scratch alone is therefore not the trigger, and
the cause is unknown -- so the gate stays and covers every group size: the per-tick class kernel and both train kernels
must compile without scratch for N = 1..8, the kernels rgb_submit launches must not spill for any N, and the class
kernel must keep its wavefronts per SIMD."""
import functools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc", path="/opt/rocm/bin") or shutil.which("hipcc")
ALL_N = (1, 2, 3, 4, 5, 6, 7, 8)


def _parse(stderr):
    out, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1); out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            out[cur][m.group(1).strip()] = int(m.group(2))
    return out


@functools.lru_cache(maxsize=None)
def segment_usage():
    """The remarks for every kernel of rgb_segment.hip: one device-only compile for the tests of the storage path
    (tests/test_segment.py, test_segment_compact.py, test_segment_flush.py), which each gate their own kernels."""
    if HIPCC is None:
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "ra_amd", "csrc", "rgb_segment.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-mllvm",
                        "-disable-machine-licm", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return _parse(r.stderr)


@pytest.fixture(scope="module")
def usage():
    """One device-only compile per group size, all eight at once (a unit per N: ~1 minute of wall clock on 8 cores
    against ~6 for the whole file in one unit)."""
    if HIPCC is None:
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "ra_amd", "csrc", "rgb_kernels.hip")
    procs = {n: subprocess.Popen([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-mllvm",
                                  "-disable-machine-licm", f"-DRGB_X_ONLY_N={n}", "-Rpass-analysis=kernel-resource-usage",
                                  "-c", src, "-o", os.devnull], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
             for n in ALL_N}
    out = {}
    for n, p in procs.items():
        _, err = p.communicate()
        assert p.returncode == 0, err[-2000:]
        out[n] = _parse(err)
    return out


def _kernel(usage, n, name):
    hits = [v for k, v in usage[n].items() if name in k]
    assert len(hits) == 1, f"{name} (N = {n}): {len(hits)} kernels match"
    return hits[0]


@pytest.mark.parametrize("n", ALL_N)
@pytest.mark.parametrize("name,max_vgprs,min_occupancy", [("rgb_tick_classes_kernelILi{n}E", 168, 3),
                                                           ("rgb_train_dealt_kernelILi{n}E", 168, 3),
                                                           ("rgb_train_kernelILi{n}E", 168, 3)])
def test_hot_kernels_use_no_scratch(usage, n, name, max_vgprs, min_occupancy):
    k = _kernel(usage, n, name.format(n=n))
    assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, f"{name.format(n=n)} spills to scratch: {k}"
    if "rgb_train_kernel" in name and n == 8:
        max_vgprs, min_occupancy = 256, 2      # (16 KiB of LDS per wavefront: ten per compute unit at best; RGB_TRAIN_PERSIST_MIN_WAVES)
    assert k["VGPRs"] <= max_vgprs, k
    assert k["Occupancy"] >= min_occupancy, k


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5))
def test_class_kernel_keeps_four_wavefronts_per_simd(usage, n):
    k = _kernel(usage, n, f"rgb_tick_classes_kernelILi{n}E")
    assert k["VGPRs"] <= 128 and k["Occupancy"] >= 4, k


@pytest.mark.parametrize("n", ALL_N)
def test_kernels_of_the_submit_path_do_not_spill(usage, n):
    """rgb_submit's rounds: the class kernel (above), the written-only kernel of rgb_submit_seq batches, the NOP tail."""
    for name in (f"rgb_tick_kernelILi{n}ELi5ELb1E",       # <N, RGB_MSG_WRITTEN, true>
                 f"rgb_tick_kernelILi{n}ELi0ELb0E"):      # <N, RGB_MSG_NOP>
        k = _kernel(usage, n, name)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, f"{name} spills to scratch: {k}"
