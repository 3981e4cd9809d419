/*
 * wal_on_cpu.cpp -- TEST INFRASTRUCTURE: ra_amd/csrc/rgb_wal.hip (checksum and framing kernels, staging,
 * validation) and rgb_wal_host.cpp compiled as x86 C++ over tests/native/fake_hip, kernels executed by the
 * fiber-per-lane block emulation of kernel_on_cpu.cpp.  The C entry points of include/ra_gpu_wal.h are exported
 * unchanged; "device" buffers are host buffers.
 */
#define RGB_HOST_EMULATION 1
#include <stdlib.h>
#include <hip/hip_runtime.h>
#ifdef RGB_EMU_OWN_RUNTIME   /* a library of this unit alone (tests/test_wal_kernels_on_cpu.py): the lane emulation comes along */
#include "emu_runtime.inc"
#endif
#ifndef RGB_EMU_FULL_API   /* stand-alone WAL build: a dummy context; with rgb_api.hip the real one is used */
struct rgb_ctx { int unused; };
extern "C" void *rgb_ctx_stream(rgb_ctx *) { return nullptr; }
extern "C" int rgb_ctx_device(rgb_ctx *) { return 0; }
#endif
#include "../../ra_amd/csrc/rgb_wal.hip"
#include "../../ra_amd/csrc/rgb_wal_host.cpp"
#ifndef RGB_EMU_FULL_API
extern "C" rgb_ctx *emu_wal_ctx() { static rgb_ctx c; return &c; }
#endif

/* rgb_seg_combine_kernel on given partial values, one workgroup as rgb_crc32_stream_device launches it: the rounds
 * behind the first (more than 256 partial values, a buffer of more than 16 MiB) without such a buffer
 * (tests/test_segment.py).  -> *crc afterwards; `crc_in` is what *crc holds before (read when init_from_crc is set) */
extern "C" uint32_t emu_seg_combine(const uint32_t *partials, uint32_t n_blocks, uint32_t xn, uint32_t init,
                                    uint32_t init_from_crc, uint32_t crc_in) {
  uint32_t crc = crc_in;
  hipLaunchKernelGGL(seg::rgb_seg_combine_kernel, dim3(1), dim3(seg::THREADS), 0, (hipStream_t) nullptr, partials,
                     n_blocks, xn, init, init_from_crc, &crc, (const unsigned char *)nullptr, 0u);
  return crc;
}
