"""Block and lane schedules of the CPU emulation (tests/native/emu_runtime.inc, emu_set_schedule): TEST PROCESS ONLY.

By default emu::launch runs workgroups 0, 1, 2, ... and, between two barriers, lanes 0 .. n-1: every atomic arrives in
index order, which no device promises.  `schedule(lib, name)` runs a block of a test under another order and always puts
ascending back.  `lib` is what owns the emulated library: the path of `emulated_kernels_so`, an `emulated_engine`, or
a ctypes library.

Nothing here touches a device: the GPU twins run the product as it is."""
import contextlib
import ctypes

ASCENDING, DESCENDING, PERMUTED, WAVEFRONTS = 0, 1, 2, 3
BLOCK_MODES = ("ascending", "descending", "permuted")
LANE_MODES = ("ascending", "descending", "permuted", "wavefronts permuted")

# name -> (block mode, lane mode, seed)
SCHEDULES = {
    "ascending": (ASCENDING, ASCENDING, 0),
    "reverse": (DESCENDING, DESCENDING, 0),
    "shuffle-1": (PERMUTED, PERMUTED, 0x5EED0001),
    "shuffle-2": (PERMUTED, PERMUTED, 0xC0FFEE02),
}
PERMUTED_SCHEDULES = ("reverse", "shuffle-1", "shuffle-2")


def setter(lib):
    """emu_set_schedule(block_mode, lane_mode, seed) of the emulated library -> the previous modes, or -1"""
    if isinstance(lib, str):
        lib = ctypes.CDLL(lib)                   # the same handle as every other CDLL of this path: one setting
    elif hasattr(lib, "lib") and callable(lib.lib):
        lib = lib.lib()                          # ra_amd.engine bound to the emulated library
    fn = lib.emu_set_schedule                    # AttributeError on the product's library: it has no such switch
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_uint64]
    return fn


@contextlib.contextmanager
def schedule(lib, name, wavefronts=False):
    """Launches inside run under the named schedule; ascending is restored whatever happens.  Whatever exception leaves
    the block carries the schedule and its seed: an AssertionError in front of its message, any other as a note.
    `wavefronts`: the lane order of the schedule becomes "the 64-lane groups permuted, ascending inside" (for a kernel
    that exchanges data inside a wavefront without a workgroup barrier -- a use has to be justified in
    profiles/mutation_audit.md).  -> the description that the messages carry."""
    block, lane, seed = SCHEDULES[name]
    if wavefronts and lane != ASCENDING:
        lane = WAVEFRONTS
    tag = "schedule %s (blocks %s, lanes %s, seed %#x)" % (name, BLOCK_MODES[block], LANE_MODES[lane], seed)
    fn = setter(lib)
    prev = fn(block, lane, seed)
    try:
        assert prev == 0, "set over a schedule that is not ascending (previous modes %#x)" % prev
        yield tag
    except AssertionError as e:
        raise AssertionError("%s: %s" % (tag, e)) from e
    except Exception as e:
        if hasattr(e, "add_note"):
            e.add_note(tag)
        else:
            e.args = e.args + (tag,)
        raise
    finally:
        fn(ASCENDING, ASCENDING, 0)
