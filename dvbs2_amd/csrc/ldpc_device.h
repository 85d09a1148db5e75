// What the LDPC kernel files (k_ldpc_wg8, k_ldpc_cu1, k_ldpc_nat, k_ldpc_lat, k_ldpc_generic) share on the device: the address-space typedefs, the packed check
// state's unpack, the exact pairing, the quad-permute exchanges and the phase timer.  One definition each; every function is forced inline (tools/isa_same.py holds
// the kernels' code to the instruction across an edit of this file).
#pragma once
#include "dvbs2hip_internal.h"

namespace dvbs2 {

// LDS pointers carry their address space in the type, so the optimiser can never merge an
// LDS access and a global access into one flat access through a selected generic pointer.
typedef __attribute__((address_space(3))) float lds_float;
typedef __attribute__((address_space(3))) int lds_int;
typedef __attribute__((address_space(3))) char lds_char;
// The layer tables are read-only for the whole launch.  Reading them through the CONSTANT
// address space lets the compiler use scalar loads (SGPRs, scalar cache) for these
// wave-uniform addresses; through a plain global pointer it must assume the kernel's own
// stores may alias them and falls back to per-lane vector loads with a full memory round
// trip in front of every edge.
typedef const __attribute__((address_space(4))) uint32_t *const_u32;
typedef const __attribute__((address_space(4))) int32_t *const_i32;
typedef const __attribute__((address_space(4))) unsigned long long *const_u64;

constexpr int LDPC_ROW = LDPC_Z * 4;        // bytes per bit-group row

// (a & m) | b in one VALU operation (the compiler emits v_and + v_or)
__device__ __forceinline__ float and_or(uint32_t a, uint32_t m_sgpr, float b)
{
    float r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(m_sgpr), "v"(b));
    return r;
}

// The min-sum kernels' storage format, packed per-check state {c1, c2, pk}: the message on slot j of a check (or half-check) with NS slots has magnitude c1 at the
// recorded minimum (pk >> 27), c2 elsewhere (both >= 0); sign = bit (NS-1-j) of pk.  `sb` = 0x80000000 held in an SGPR.
template <int NS>
__device__ __forceinline__ float ldpc_unpack(float c1, float c2, uint32_t pk, uint32_t j, uint32_t sb)
{
    const float mag = ((pk >> 27) == j) ? c1 : c2;
    return and_or(pk << ((32u - NS) + j), sb, mag);
}

// exact sum-product pairing (`--dec-implem SPA`, the reference's default), as the oracle's chk_update_spa:
//     a [+] b = sign(a) sign(b) min(|a|,|b|) + log(1 + e^-|a+b|) - log(1 + e^-|a-b|)
// on the hardware exp2 / log2 units.  +inf is the neutral element (absent / NULL slots carry it).
// CHECKED = false: at most one operand is +inf (regular codes: only the absent edge of lane 0 carries it), for which the
// formula itself returns the other operand (e^-inf = 0); CHECKED = true (padded layers, several +inf slots in a row): the
// inf - inf of two neutral elements is caught by selects.
template <bool CHECKED>
__device__ __forceinline__ float ldpc_boxplus(float a, float b)
{
    const float e1 = __builtin_amdgcn_exp2f(-1.44269504088896341f * fabsf(a + b)), e2 = __builtin_amdgcn_exp2f(-1.44269504088896341f * fabsf(a - b));
    const float l = (__builtin_amdgcn_logf(1.0f + e1) - __builtin_amdgcn_logf(1.0f + e2)) * 0.693147180559945309f;
    const float mn = fminf(fabsf(a), fabsf(b));
    const float sg = __uint_as_float((__float_as_uint(mn) & 0x7FFFFFFFu) | ((__float_as_uint(a) ^ __float_as_uint(b)) & 0x80000000u));
    if (!CHECKED) return sg + l;
    return a == INFINITY ? b : (b == INFINITY ? a : sg + l);
}

// the value of the neighbouring lane inside a quad (DPP, no LDS): lane ^ 1 and lane ^ 2
__device__ __forceinline__ float quad_xor1(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)); }      // quad_perm [1,0,3,2]
__device__ __forceinline__ uint32_t quad_xor1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ float quad_xor2(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)); }      // quad_perm [2,3,0,1]

// development aid (-DLDPC_PHASE_PROF): the ticks since the last mark go to the wave's phase slot i (`prof`, `pt_` are the kernel's)
#ifdef LDPC_PHASE_PROF
#define LDPC_PROF_MARK(i) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); prof[i] += (uint32_t)(n_ - pt_); pt_ = n_; } while (0)
#else
#define LDPC_PROF_MARK(i)
#endif

}  // namespace dvbs2
