// fsk_bytesel.h — the byte-select add, the half-select xor, the first-use point of LDS reads and the LDS-only barrier of the
// packed shift corrections (k_dense_shift_packed, fsk_kernels_dense_shift.h).
//
// acc + byte B of `packed` is ONE v_add_u32_sdwa on gfx950 (src0_sel:BYTE_B); written in C++ hipcc emits v_bfe_u32 + v_add3_u32
// for two cells, one and a half instructions a cell in a kernel that is bound by the VALU instructions it issues.
//
// Why this header holds its own FSK_EMU branch, unlike fsk_gfx950.h: the CPU emulation of the test-suite (tests/emu/hip_emu.h)
// provides the functions of fsk_gfx950.h under the same names and belongs to the existing tests, which stay as they are. It has
// no byte-select add and no first-use point, so the plain-C++ bodies the emulated build compiles live here, beside the instructions
// they stand for.
#pragma once
#include "fsk_platform.h"

namespace fsk_hw {

// (volatile: the adds keep their place between the first-use points below, which is what orders a step's work around its waits)
template <int B>
__device__ __forceinline__ uint32_t add_byte(uint32_t acc, uint32_t packed) {
    static_assert(B >= 0 && B < 4, "a dword has four bytes");
#ifdef FSK_EMU
    return acc + ((packed >> (8 * B)) & 255u);
#else
    uint32_t d;
    if constexpr (B == 0)
        asm volatile("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(acc));
    else if constexpr (B == 1)
        asm volatile("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(acc));
    else if constexpr (B == 2)
        asm volatile("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(acc));
    else
        asm volatile("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(acc));
    return d;
#endif
}

// 16-bit half W of `packed`, zero-extended, xor x: ONE v_xor_b32_sdwa (src0_sel:WORD_W). The kernel keeps two 14-bit LDS offsets
// in a dword and xors a lane term and the stage's base into both: xor, mask and xor, shift in C++ — three instructions a pair.
template <int W>
__device__ __forceinline__ uint32_t xor_word(uint32_t packed, uint32_t x) {
    static_assert(W == 0 || W == 1, "a dword has two halves");
#ifdef FSK_EMU
    return ((packed >> (16 * W)) & 0xffffu) ^ x;
#else
    uint32_t d;
    if constexpr (W == 0)
        asm("v_xor_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(x));
    else
        asm("v_xor_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(x));
    return d;
#endif
}

// The point in a kernel at which eight LDS reads are FIRST USED, all together: an empty instruction that takes and returns the
// eight registers. Nothing computed from them can be scheduled before it, and no memory access can be moved across it, so the
// reads issued before it stay in flight up to here and the ones issued after it are under way while the eight are worked on. The
// compiler places the one counted wait (s_waitcnt lgkmcnt(N), N = the reads issued later) in front of it. Left to itself hipcc
// moves the first instruction of every use up to its read and drains the counter pair by pair.
__device__ __forceinline__ void first_use(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t& e, uint32_t& f, uint32_t& g, uint32_t& h) {
#ifndef FSK_EMU
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h) : : "memory");
#endif
}

// A workgroup barrier that orders LDS accesses only: s_waitcnt lgkmcnt(0) + s_barrier, and no wait on the vector-memory
// counter. __syncthreads() is a workgroup fence as well and drains vmcnt, which ends a direct-to-LDS load that is meant to stay
// in flight across the barrier (the ahead schedule of k_dense_shift_packed). Everything the waves exchange through LDS by
// ds_read / ds_write / ds_add is ordered by it; what a direct-to-LDS load lands is NOT: that needs fsk_hw::wait_panel_rows()
// in front of a barrier.
__device__ __forceinline__ void barrier_lds_only() {
#ifdef FSK_EMU
    __syncthreads();
#else
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}

}  // namespace fsk_hw
