// fsk_exp_neg.h — exp(x) for x <= 0 as a FIXED SEQUENCE OF IEEE OPERATIONS: the same bits on the host and on the device,
// whatever libm or the device library would give. Used where a probability must be restated bit for bit (k_svm_ovo_proba's
// sigmoids); the host has it as fsk_exp_neg of include/fastsk_amd.h. This file is built without contraction like the rest of
// the SVM code: every multiply and every add below is one rounding (__dmul_rn / __dadd_rn / __dsub_rn on the device).
//
//   NaN -> NaN (the argument itself); x > 0 is not supported (no caller passes it); x < -708 -> 0.0, so that no subnormal is
//   ever formed (exp(-708) = 3.3e-308 is normal). Otherwise
//   n = floor(x * (1 / ln 2) + 0.5)                      -1021 <= n <= 0
//   r = (x - n * LN2_HI) - n * LN2_LO                    Cody-Waite: LN2_HI has 32 trailing zero bits, n * LN2_HI is exact
//   q = 1/13!; q = q * r + 1/i! for i = 12 .. 0          Horner, one multiply and one add a step, |r| <= 0.347
//   the result is q * 2^n, 2^n built from its exponent bits: exact, n >= -1022.
// Measured against libm's exp (tests/test_emu_svm_multiclass_proba.py): at most 1 ulp on [-708, 0]; the design's bound is 2.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIP_DEVICE_COMPILE__)
#define FSK_EXP_MUL(a, b) __dmul_rn((a), (b))
#define FSK_EXP_ADD(a, b) __dadd_rn((a), (b))
#define FSK_EXP_SUB(a, b) __dsub_rn((a), (b))
#define FSK_EXP_FLOOR(a) floor(a)
#else
#define FSK_EXP_MUL(a, b) ((a) * (b))
#define FSK_EXP_ADD(a, b) ((a) + (b))
#define FSK_EXP_SUB(a, b) ((a) - (b))
#define FSK_EXP_FLOOR(a) __builtin_floor(a)
#endif

namespace fsk {

__host__ __device__ inline double exp_neg(double x) {
    constexpr double INV_LN2 = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33;
    if (x != x) return x;
    if (x < -708.0) return 0.0;
    const double n = FSK_EXP_FLOOR(FSK_EXP_ADD(FSK_EXP_MUL(x, INV_LN2), 0.5));
    const double r = FSK_EXP_SUB(FSK_EXP_SUB(x, FSK_EXP_MUL(n, LN2_HI)), FSK_EXP_MUL(n, LN2_LO));
    double q = 1.0 / 6227020800.0;                         // 1 / 13!
    q = FSK_EXP_ADD(FSK_EXP_MUL(q, r), 1.0 / 479001600.0);  // 1 / 12!
    q = FSK_EXP_ADD(FSK_EXP_MUL(q, r), 1.0 / 39916800.0);
    q = FSK_EXP_ADD(FSK_EXP_MUL(q, r), 1.0 / 3628800.0);
    q = FSK_EXP_ADD(FSK_EXP_MUL(q, r), 1.0 / 362880.0);
    q = FSK_EXP_ADD(FSK_EXP_MUL(q, r), 1.0 / 40320.0);
    q = FSK_EXP_ADD(FSK_EXP_MUL(q, r), 1.0 / 5040.0);
    q = FSK_EXP_ADD(FSK_EXP_MUL(q, r), 1.0 / 720.0);
    q = FSK_EXP_ADD(FSK_EXP_MUL(q, r), 1.0 / 120.0);
    q = FSK_EXP_ADD(FSK_EXP_MUL(q, r), 1.0 / 24.0);
    q = FSK_EXP_ADD(FSK_EXP_MUL(q, r), 1.0 / 6.0);
    q = FSK_EXP_ADD(FSK_EXP_MUL(q, r), 0.5);
    q = FSK_EXP_ADD(FSK_EXP_MUL(q, r), 1.0);
    q = FSK_EXP_ADD(FSK_EXP_MUL(q, r), 1.0);
    const uint64_t bits = (uint64_t)((int64_t)n + 1023) << 52;  // 2^n: a biased exponent of 2 .. 1023, no mantissa bits
    double scale;
    memcpy(&scale, &bits, sizeof scale);
    return FSK_EXP_MUL(q, scale);
}

}  // namespace fsk

#undef FSK_EXP_MUL
#undef FSK_EXP_ADD
#undef FSK_EXP_SUB
#undef FSK_EXP_FLOOR
