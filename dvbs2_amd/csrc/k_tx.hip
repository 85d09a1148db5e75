// N1 -- TX mirror + AWGN channel on the device, so the Monte-Carlo BER loop of
// dvbs2_tx_rx_bb (/root/reference src/mains/TX_RX_BB/main.cpp:75-82) never leaves the GPU:
//   source.generate -> bb_scrambler.scramble -> BCH encode (Encoder_BCH_DVBS2.cpp:28-43)
//   -> LDPC encode (enc type "LDPC_DVBS2", DVBS2.cpp:427) -> interleave (DVBS2.cpp:451-476)
//   -> modulate (Modem_generic) -> Framer::generate (Framer.hxx:232-293)
//   -> Scrambler_PL::scramble (Scrambler_PL.hxx:61-78) -> Channel_AWGN (DVBS2.cpp:593-613)
// Test-signal generation, not the RX hot path; parity: bit-exact against the oracle TX for
// given payloads and sigma = 0 (tests/test_tx_gpu.py).  Noise: Philox4x32-10 + Box-Muller,
// counter = (symbol, frame, stream), so results do not depend on the launch geometry.
#include "dvbs2hip_internal.h"
#include "rx_device.h"
#include "tx_encoders.h"

namespace dvbs2 {

// ---------------------------------------------------------------- Philox4x32-10
__device__ __forceinline__ uint4 philox4x32(uint4 ctr, uint2 key)
{
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * ctr.x;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * ctr.z;
        ctr = make_uint4((uint32_t)(p1 >> 32) ^ ctr.y ^ key.x, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ ctr.w ^ key.y, (uint32_t)p0);
        key.x += 0x9E3779B9u; key.y += 0xBB67AE85u;
    }
    return ctr;
}

// ---------------------------------------------------------------- source + BB scramble (coalesced, one workgroup per frame)
__global__ void __launch_bounds__(256)
tx_src_kernel(const TxKParams p)
{
    extern __shared__ uint32_t wsm[];                          // payload, packed
    const int f = blockIdx.x, tid = threadIdx.x, K = p.K_bch;
    const int nwk = (K + 31) / 32, nw_out = (p.K_ldpc + 31) / 32;
    for (int w = tid; w < nwk; w += 256) {
        uint32_t word = 0u;
        if (p.info_in) {
            const int32_t *src = p.info_in + (size_t)f * K + 32 * w;
            for (int b = 0; b < 32 && 32 * w + b < K; b++) word |= ((uint32_t)src[b] & 1u) << b;
        } else {
            const uint4 r = philox4x32(make_uint4((uint32_t)(w >> 2), (uint32_t)f, 0u, 0u), make_uint2(p.seed_lo, p.seed_hi));
            word = (w & 3) == 0 ? r.x : (w & 3) == 1 ? r.y : (w & 3) == 2 ? r.z : r.w;
            if (32 * w + 32 > K) word &= (1u << (K - 32 * w)) - 1u;
        }
        wsm[w] = word;
        p.bch_cw[(size_t)f * nw_out + w] = word ^ p.prbs[w];    // Scrambler_BB (prbs tail bits are zero)
    }
    __syncthreads();
    if (p.info_out)
        for (int k = tid; k < K; k += 256) p.info_out[(size_t)f * K + k] = (int32_t)((wsm[k >> 5] >> (k & 31)) & 1u);
}

// ---------------------------------------------------------------- BCH parity (Encoder_BCH_DVBS2.cpp:28-43)
// The segmented division: tx_bch_remainder (tx_encoders.h).  Lane seg == 0 of a frame appends the parity at bit K of the packed frame.
__global__ void __launch_bounds__(64)
tx_bchpar_kernel(const TxKParams p)
{
    __shared__ unsigned long long T[256][3];
    __shared__ uint8_t brev[256];
    const TxBchRem R = tx_bch_remainder(p, T, brev);
    if (!R.live || R.seg != 0) return;
    const int K = p.K_bch, r = p.K_ldpc - p.K_bch;
    const int nw_out = (p.K_ldpc + 31) / 32;
    uint32_t *cw = p.bch_cw + (size_t)R.f * nw_out;
    uint32_t outw = (K & 31) ? cw[K >> 5] : 0u;
    for (int j = 0; j < r; j++) {
        const int k = K + j;
        outw |= tx_bch_parity_bit(R, r, j) << (k & 31);
        if ((k & 31) == 31) { cw[k >> 5] = outw; outw = 0; }
    }
    if ((p.K_ldpc & 31) != 0) cw[nw_out - 1] = outw;
}

// ---------------------------------------------------------------- LDPC IRA encoder (ETSI EN 302 307 5.3.2)
// One workgroup per frame: the packed information bits and the layer table into LDS, tx_ldpc_rows (tx_encoders.h) forms the parity rows and the column prefix there, and a
// lane packs one word of the code word.
__global__ void __launch_bounds__(LDPC_THREADS)
tx_ldpc_kernel(const TxKParams p)
{
    extern __shared__ uint32_t sm[];
    const int K = p.K_ldpc, q = (p.N_ldpc - p.K_ldpc) / LDPC_Z;
    const int nw_in = (K + 31) / 32, nw_out = (p.N_ldpc + 31) / 32;
    const TxLdpcLds L = tx_ldpc_lds(sm, p);
    const int t = threadIdx.x, f = blockIdx.x;
    for (int w = t; w < q * p.enc_stride; w += LDPC_THREADS) L.tab[w] = p.enc_tab[w];
    const uint32_t *src = p.bch_cw + (size_t)f * nw_in;
    for (int w = t; w <= nw_in; w += LDPC_THREADS) L.info[w] = w < nw_in ? src[w] : 0u;
    __syncthreads();
    tx_ldpc_rows(p, L, t);
    __syncthreads();
    uint32_t *dst = p.ldpc_cw + (size_t)f * nw_out;
    for (int w = t; w < nw_out; w += LDPC_THREADS) {
        uint32_t word = 0;
        const int i0 = 32 * w;
        if (i0 + 32 <= K) word = L.info[w];                   // systematic part, word-aligned
        else {
            // parity bit c = i - K sits at (r = c mod q, tt = c / q): stepped, one division per word
            int c = i0 >= K ? i0 - K : 0, tt = c / q, r = c - tt * q;
            for (int b = 0; b < 32; b++) {
                const int i = i0 + b;
                if (i >= p.N_ldpc) break;
                uint32_t bit;
                if (i < K) bit = (L.info[i >> 5] >> (i & 31)) & 1u;
                else { bit = tx_ldpc_parity_bit(L, r, tt); if (++r == q) { r = 0; tt++; } }
                word |= bit << b;
            }
        }
        dst[w] = word;
    }
}

// ---------------------------------------------------------------- interleave + modulate + frame + PL scramble + AWGN
// One lane per PAIR of PL symbols: one Philox4x32-10 block (four words) is exactly the two Box-Muller pairs the two symbols
// need, and the lane leaves with one 16-byte store.
// BPS > 0: bits per symbol known at compile time (the bit gathers of a symbol are issued together, not one dependent load
// after the other) and, with ITL, the column/row interleaver with as many columns as bits per symbol (every DVB-S2 one):
// interleaved bit k bps + b sits at natural position col(b) * n_rows + k -- no division.  BPS == 0: any configuration.
template <int BPS, bool ITL>
__device__ __forceinline__ float2 tx_symbol(const TxKParams &p, const float *cs, const uint32_t *cw, int i, int n_pil)
{
    // Branch-free for the compile-time BPS forms: header, pilot and data symbols take the same instructions (indices clamped, the
    // right value selected at the end) -- a wave nearly always holds one kind only, but every branch costs the scalar unit a
    // save / restore of the execution mask, and there were seventy of those per pair of symbols.
    // inverse of the RX map: position i-90 inside [16 slots data | 36 pilots] blocks
    const int j = i >= PL_M ? i - PL_M : 0, blk = j / (PL_GAP + PL_P), off = j - blk * (PL_GAP + PL_P);
    const bool pilot = blk < n_pil && off >= PL_GAP;
    int k = blk < n_pil ? blk * PL_GAP + off : n_pil * PL_GAP + (j - n_pil * (PL_GAP + PL_P));
    float2 y;
    if (BPS > 0) {
        k = pilot ? 0 : k;                                           // (any valid symbol: its value is not used)
        const int n_rows = p.N_ldpc / BPS;
        uint32_t wd[BPS > 0 ? BPS : 1];
#pragma unroll
        for (int b = 0; b < BPS; b++) {
            const int nat = ITL ? (p.itl_order == 0 ? b : BPS - 1 - b) * n_rows + k : k * BPS + b;
            wd[b] = cw[nat >> 5] >> (nat & 31);
        }
        int idx = 0;
#pragma unroll
        for (int b = 0; b < BPS; b++) idx |= (int)(wd[b] & 1u) << b;
        y = make_float2(cs[2 * idx], cs[2 * idx + 1]);
        if (pilot) y = make_float2(0.70710678118654752440f, 0.70710678118654752440f);     // pilot (Framer.hxx:252-260)
    } else if (pilot) y = make_float2(0.70710678118654752440f, 0.70710678118654752440f);
    else {
        int idx = 0;
        for (int b = 0; b < p.bps; b++) {
            // interleaved bit k*bps+b comes from natural position col*n_rows + row (column/row interleaver)
            int nat = k * p.bps + b;
            if (p.itl_cols > 1) { const int row = nat / p.itl_cols, c = nat - row * p.itl_cols; nat = (p.itl_order == 0 ? c : p.itl_cols - 1 - c) * (p.N_ldpc / p.itl_cols) + row; }
            idx |= (int)((cw[nat >> 5] >> (nat & 31)) & 1u) << b;
        }
        y = make_float2(cs[2 * idx], cs[2 * idx + 1]);
    }
    // multiply by exp(j pi/2 R) (Scrambler_PL.hxx:66-76, scr_flag = true): R = 1: (-y, x), 2: (-x, -y), 3: (y, -x) -- a swap and sign flips
    const int R = p.pl_seq[j] & 3;
    const float a = (R & 1) ? -y.y : y.x, b = (R & 1) ? y.x : y.y;
    y = (R & 2) ? make_float2(-a, -b) : make_float2(a, b);
    const int ih = i < PL_M ? i : 0;
    const float2 h = make_float2(p.plh[2 * ih], p.plh[2 * ih + 1]);   // the PL header is neither scrambled nor modulated here
    return i < PL_M ? h : y;
}

constexpr int TX_MOD_U = 4;                               // pairs of PL symbols per lane (independent: their loads overlap)
template <int BPS, bool ITL>
__global__ void __launch_bounds__(256)
tx_mod_kernel(const TxKParams p)
{
    __shared__ float cs[64];
    const int f = blockIdx.y;
    if (threadIdx.x < (2 << p.bps)) cs[threadIdx.x] = p.cstl[threadIdx.x];
    __syncthreads();
    const int n_pil = p.n_sym / PL_GAP;
    const uint32_t *cw = p.ldpc_cw + (size_t)f * ((p.N_ldpc + 31) / 32);
    const float sg = p.sigma ? p.sigma[f] : 0.f;
#pragma unroll
    for (int u = 0; u < TX_MOD_U; u++) {
        const int pr = (blockIdx.x * TX_MOD_U + u) * blockDim.x + threadIdx.x;     // pair of PL symbols 2 pr, 2 pr + 1
        const int i0 = 2 * pr;
        if (i0 >= p.pl_frame) continue;
        const bool two = i0 + 1 < p.pl_frame;
        float2 y0 = tx_symbol<BPS, ITL>(p, cs, cw, i0, n_pil), y1 = two ? tx_symbol<BPS, ITL>(p, cs, cw, i0 + 1, n_pil) : make_float2(0.f, 0.f);
        if (sg != 0.f) {                                             // (sigma = 0 is the noiseless frame bit for bit: adding 0 * n would turn a -0 of the constellation into +0)
            const uint4 r = philox4x32(make_uint4((uint32_t)pr, (uint32_t)f, 1u, 0u), make_uint2(p.seed_lo, p.seed_hi));
            // Box-Muller on the hardware units: v_log_f32, v_sqrt_f32, and v_sin_f32 / v_cos_f32, which take their argument in
            // revolutions (u2 itself) -- the accurate libm forms cost ~10x the instructions and the noise needs none of it
            const float u1 = ((float)r.x + 1.0f) * 2.3283064365386963e-10f, u2 = (float)r.y * 2.3283064365386963e-10f;
            const float u3 = ((float)r.z + 1.0f) * 2.3283064365386963e-10f, u4 = (float)r.w * 2.3283064365386963e-10f;
            const float ra = sg * __builtin_amdgcn_sqrtf(-2.0f * hw_log(u1)), rb = sg * __builtin_amdgcn_sqrtf(-2.0f * hw_log(u3));
            y0.x += ra * __builtin_amdgcn_cosf(u2); y0.y += ra * __builtin_amdgcn_sinf(u2);
            y1.x += rb * __builtin_amdgcn_cosf(u4); y1.y += rb * __builtin_amdgcn_sinf(u4);
        }
        float2 *out = reinterpret_cast<float2 *>(p.pl_out + (size_t)f * 2 * p.pl_frame) + i0;
        if (two && ((reinterpret_cast<uintptr_t>(out) & 15) == 0)) *reinterpret_cast<float4 *>(out) = make_float4(y0.x, y0.y, y1.x, y1.y);
        else { out[0] = y0; if (two) out[1] = y1; }
    }
}

// Channel_AWGN::add_noise (DVBS2.cpp:593-613): Y = X + sigma[f] * n, n ~ N(0,1) per real value.
// Philox counter = (pair index, frame, stream 2): independent of the launch geometry.
__global__ void awgn_kernel(const float2 *x, float2 *y, const float *sigma, uint32_t seed_lo, uint32_t seed_hi, long long n_pairs)
{
    const int f = blockIdx.y;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    const float sg = sigma[f];
    const float2 v = x[(size_t)f * n_pairs + i];
    if (sg == 0.f) { y[(size_t)f * n_pairs + i] = v; return; }          // the frame itself, bit for bit (v + 0 * n would turn -0 into +0)
    const uint4 r = philox4x32(make_uint4((uint32_t)i, (uint32_t)f, 2u, (uint32_t)(i >> 32)), make_uint2(seed_lo, seed_hi));
    const float u1 = ((float)r.x + 1.0f) * 2.3283064365386963e-10f, u2 = (float)r.y * 2.3283064365386963e-10f;
    const float rad = sg * __builtin_amdgcn_sqrtf(-2.0f * hw_log(u1));
    const float sn = __builtin_amdgcn_sinf(u2), cn = __builtin_amdgcn_cosf(u2);
    y[(size_t)f * n_pairs + i] = make_float2(v.x + rad * cn, v.y + rad * sn);
}
hipError_t awgn_launch(const float *x, float *y, const float *sigma, unsigned long long seed, long long n_pairs, int F, hipStream_t s)
{
    hipLaunchKernelGGL(awgn_kernel, dim3((unsigned)((n_pairs + 255) / 256), F), dim3(256), 0, s, reinterpret_cast<const float2 *>(x),
                       reinterpret_cast<float2 *>(y), sigma, (uint32_t)seed, (uint32_t)(seed >> 32), n_pairs);
    return hipGetLastError();
}

hipError_t tx_launch(const TxKParams &p, hipStream_t s)
{
    hipLaunchKernelGGL(tx_src_kernel, dim3(p.n_frames), dim3(256), (size_t)((p.K_bch + 31) / 32) * 4, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tx_bchpar_kernel, dim3((p.n_frames + 64 / TX_BCH_SEG - 1) / (64 / TX_BCH_SEG)), dim3(64), 0, s, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tx_ldpc_kernel, dim3(p.n_frames), dim3(LDPC_THREADS), tx_ldpc_lds_bytes(p), s, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 g(((p.pl_frame + 1) / 2 + 256 * TX_MOD_U - 1) / (256 * TX_MOD_U), p.n_frames), b(256);
    const bool itl = p.itl_cols > 1;
    if (itl && p.itl_cols != p.bps) hipLaunchKernelGGL((tx_mod_kernel<0, false>), g, b, 0, s, p);          // not a DVB-S2 interleaver: general form
    else if (p.bps == 1) hipLaunchKernelGGL((tx_mod_kernel<1, false>), g, b, 0, s, p);
    else if (p.bps == 2 && !itl) hipLaunchKernelGGL((tx_mod_kernel<2, false>), g, b, 0, s, p);
    else if (p.bps == 2) hipLaunchKernelGGL((tx_mod_kernel<2, true>), g, b, 0, s, p);
    else if (p.bps == 3 && !itl) hipLaunchKernelGGL((tx_mod_kernel<3, false>), g, b, 0, s, p);
    else if (p.bps == 3) hipLaunchKernelGGL((tx_mod_kernel<3, true>), g, b, 0, s, p);
    else if (p.bps == 4 && itl) hipLaunchKernelGGL((tx_mod_kernel<4, true>), g, b, 0, s, p);
    else if (p.bps == 5 && itl) hipLaunchKernelGGL((tx_mod_kernel<5, true>), g, b, 0, s, p);
    else hipLaunchKernelGGL((tx_mod_kernel<0, false>), g, b, 0, s, p);
    return hipGetLastError();
}

}  // namespace dvbs2
