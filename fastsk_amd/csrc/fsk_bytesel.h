// fsk_bytesel.h — the byte-select add of the packed shift corrections (k_dense_shift_packed, fsk_kernels_dense_shift.h).
//
// acc + byte B of `packed` is ONE v_add_u32_sdwa on gfx950 (src0_sel:BYTE_B); written in C++ hipcc emits v_bfe_u32 + v_add3_u32
// for two cells, one and a half instructions a cell in a kernel that is bound by the VALU instructions it issues.
//
// Why this header holds its own FSK_EMU branch, unlike fsk_gfx950.h: the CPU emulation of the test-suite (tests/emu/hip_emu.h)
// provides the functions of fsk_gfx950.h under the same names and belongs to the existing tests, which stay as they are. It has
// no byte-select add, so the plain-C++ body the emulated build compiles lives here, beside the instruction it stands for.
#pragma once
#include "fsk_platform.h"

namespace fsk_hw {

template <int B>
__device__ __forceinline__ uint32_t add_byte(uint32_t acc, uint32_t packed) {
    static_assert(B >= 0 && B < 4, "a dword has four bytes");
#ifdef FSK_EMU
    return acc + ((packed >> (8 * B)) & 255u);
#else
    uint32_t d;
    if constexpr (B == 0)
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(acc));
    else if constexpr (B == 1)
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(acc));
    else if constexpr (B == 2)
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(acc));
    else
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(d) : "v"(packed), "v"(acc));
    return d;
#endif
}

}  // namespace fsk_hw
