// What the kernel files outside the LDPC decoder share on the device (k_front, k_pls, k_est_pilots; the PL-frame geometry also k_tx, k_tx_tasks and api_est_pilots): the
// layout of a PL frame, the PL derotation, the cross-lane moves of a wave, and the noise estimators' last step.  One
// definition each; every function is forced inline (tools/isa_same.py holds the kernels' code to the instruction across an edit of this file).  The counterpart of
// ldpc_device.h.  The constants are plain constexpr and serve host code too; everything else is device code.
#pragma once
#include "dvbs2hip_internal.h"

namespace dvbs2 {

// ---------------------------------------------------------------- PL-frame geometry (Framer.hxx:232-293)
// PL frame = PL_M header symbols | [PL_SLOTS slots of PL_M data symbols | PL_P pilots] x n_pilots | the remaining data
constexpr int PL_M = 90, PL_P = 36, PL_SLOTS = 16;
constexpr int PL_GAP = PL_SLOTS * PL_M;              // 1440 data symbols between two pilot blocks

// xfec symbol k -> index of the same symbol inside the PL frame (Framer.hxx:330-343)
__device__ __forceinline__ int pl_index(int k, int n_pilots)
{
    int b = k / PL_GAP;
    b = b < n_pilots ? b : n_pilots;
    return PL_M + k + PL_P * b;
}

// known symbol k of the L = PL_M + PL_P n_pilots a receiver knows (k < PL_M: the header; k = PL_M + PL_P b + i: pilot i of block b) -> its index inside the PL frame
__device__ __forceinline__ int pl_known_index(int k)
{
    return k >= PL_M ? k + PL_GAP * ((k - PL_M) / PL_P + 1) : k;
}

// multiply by conj(exp(j pi/2 R)) (Scrambler_PL.hxx:66-76 with scr_flag = false)
__device__ __forceinline__ float2 pl_derotate(float2 x, int R)
{
    // R = 0: (x, y)   1: (y, -x)   2: (-x, -y)   3: (-y, x) -- branch-free (a switch becomes four exec-masked paths per wave, every wave holds all four values):
    // odd R swaps the parts, bit 1 of R negates the first output, bit 1 of R + 1 the second
    const bool sw = (R & 1) != 0;
    const float a = sw ? x.y : x.x, b = sw ? x.x : x.y;
    return make_float2(__uint_as_float(__float_as_uint(a) ^ (((uint32_t)R << 30) & 0x80000000u)), __uint_as_float(__float_as_uint(b) ^ (((uint32_t)(R + 1) << 30) & 0x80000000u)));
}

// ---------------------------------------------------------------- cross-lane moves
// the value of lane (l ^ M)
template <int M> __device__ __forceinline__ float wave_xor(float v)
{
    const int x = __builtin_bit_cast(int, v);
    int r;
    if constexpr (M == 1) r = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true);            // quad_perm [1,0,3,2]
    else if constexpr (M == 2) r = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true);       // quad_perm [2,3,0,1]
    else if constexpr (M == 8) r = __builtin_amdgcn_update_dpp(0, x, 0x128, 0xF, 0xF, true);      // row_ror:8
    else if constexpr (M == 4 || M == 16) r = __builtin_amdgcn_ds_swizzle(x, 0x1F | (M << 10));   // bit mode: and 0x1F, or 0, xor M, inside each half of the wave
    else r = __builtin_amdgcn_ds_bpermute((int)((__lane_id() ^ M) << 2), x);
    return __builtin_bit_cast(float, r);
}
template <int M> __device__ __forceinline__ uint32_t wave_xor(uint32_t v) { return __builtin_bit_cast(uint32_t, wave_xor<M>(__builtin_bit_cast(float, v))); }
// all-reduce over the 64 lanes in six xor steps: every lane ends with the same sum
__device__ __forceinline__ float wave_sum(float v)
{
    v = v + wave_xor<1>(v); v = v + wave_xor<2>(v); v = v + wave_xor<4>(v); v = v + wave_xor<8>(v); v = v + wave_xor<16>(v); v = v + wave_xor<32>(v);
    return v;
}

// ---------------------------------------------------------------- noise estimators
// Es/N0 [dB] -> sigma and Eb/N0 (Estimator_DVBS2.hxx:54-56), the last step of the M2M4 estimator (k_front.hip) and of the pilot-aided one (k_est_pilots.hip), on the
// hardware units (see m2m4_finish).  rate_bps = code rate x bits per symbol
__device__ __forceinline__ void esn0_to_sigma_ebn0(float esn0, float rate_bps, float &sigma, float &ebn0)
{
    sigma = __builtin_amdgcn_sqrtf(__builtin_amdgcn_rcpf(2.0f * __builtin_amdgcn_exp2f(esn0 * 0.332192809488736f)));      // sqrt(1 / (2 10^(esn0 / 10)))
    ebn0 = esn0 - 10.f * 0.301029995663981f * __builtin_amdgcn_logf(rate_bps);
}

}  // namespace dvbs2
