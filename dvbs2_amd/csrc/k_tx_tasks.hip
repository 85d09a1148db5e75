// The transmitter's tasks at the task boundary: one kernel (the BCH encoder: two) per codelet the reference's TX mains bind between the source and
// the shaping filter (src/mains/TX/main.cpp:70-78 of the reference), sockets as the reference has them -- one int32 per bit, one pair of floats per
// symbol:
//   Encoder_BCH_DVBS2::encode (Encoder_BCH_DVBS2.cpp:28-43) -> LDPC encode (DVBS2.cpp:427) -> Interleaver::interleave (DVBS2.cpp:451-476)
//   -> Modem::modulate (Modem_generic) -> Framer::generate (Framer.hxx:232-293) -> Scrambler_PL::scramble (Scrambler_PL.hxx:61-78)
// (Scrambler_BB::scramble is the XOR of its inverse: bb_descramble_kernel, k_front.hip).  The arithmetic is the fused TX mirror's (k_tx.hip; the
// encoders' is tx_encoders.h, which both files call); what is new is the socket form.  Every task is a streaming pass: the input is read once, the output written once,
// 16 bytes per lane where the socket's address and the frame size allow it (`vec`, decided by the launcher for the whole grid) and 4 / 8 bytes per
// access otherwise.  Two input sides are 4-byte loads whatever the alignment: the interleaver's gather (a lane's four bits lie in different columns) and the
// modulator's bits (2 bps of them per lane, 16-byte aligned only for bps 2 and 4); their stores are 16 bytes.  Grids as the stand-alone front-end kernels of k_front.hip: 256 lanes per workgroup along the frame, the frame in blockIdx.y.
#include "dvbs2hip_internal.h"
#include "rx_device.h"
#include "tx_encoders.h"

namespace dvbs2 {

typedef int txt_i4 __attribute__((ext_vector_type(4)));

__host__ __device__ __forceinline__ bool txt_al16(const void *a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

// bits i .. i + 3 of a frame of n (what lies behind the frame reads as 0); vec: i + 4 <= n or i >= n, and the address is 16-byte aligned
__device__ __forceinline__ txt_i4 txt_load4(const int32_t *__restrict__ src, int i, int n, bool vec)
{
    txt_i4 v = {0, 0, 0, 0};
    if (vec) { if (i < n) v = *reinterpret_cast<const txt_i4 *>(src + i); }
    else {
        if (i < n) v.x = src[i];
        if (i + 1 < n) v.y = src[i + 1];
        if (i + 2 < n) v.z = src[i + 2];
        if (i + 3 < n) v.w = src[i + 3];
    }
    return v & 1;
}
__device__ __forceinline__ void txt_store4(int32_t *__restrict__ dst, int i, int n, bool vec, txt_i4 v)
{
    if (vec) { if (i < n) *reinterpret_cast<txt_i4 *>(dst + i) = v; }
    else {
        if (i < n) dst[i] = v.x;
        if (i + 1 < n) dst[i + 1] = v.y;
        if (i + 2 < n) dst[i + 2] = v.z;
        if (i + 3 < n) dst[i + 3] = v.w;
    }
}

// 8 bits -> bit k at position 4 k
__device__ __forceinline__ uint32_t txt_spread4(uint32_t x)
{
    x = (x | (x << 12)) & 0x000F000Fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = (x | (x << 3)) & 0x11111111u;
    return x;
}
// A wave packs 256 consecutive bits: lane l holds bits 4 l .. 4 l + 3 (one 16-byte load).  Four ballots give, for j = 0 .. 3, the 64-bit mask of
// bit 4 l + j over the lanes; packed word w = bits 32 w .. 32 w + 31 = lanes 8 w .. 8 w + 7, i.e. byte w of every mask with its bits spread to
// every fourth position.  Lane w < 8 returns word w (the other lanes a word nobody uses).  Called by whole waves only.
__device__ __forceinline__ uint32_t txt_pack256(txt_i4 b, int lane)
{
    const unsigned long long m0 = __ballot(b.x != 0), m1 = __ballot(b.y != 0), m2 = __ballot(b.z != 0), m3 = __ballot(b.w != 0);
    const int sh = 8 * (lane & 7);
    return txt_spread4((uint32_t)(m0 >> sh) & 0xFFu) | (txt_spread4((uint32_t)(m1 >> sh) & 0xFFu) << 1) |
           (txt_spread4((uint32_t)(m2 >> sh) & 0xFFu) << 2) | (txt_spread4((uint32_t)(m3 >> sh) & 0xFFu) << 3);
}

// ---------------------------------------------------------------- BCH encode, 1 of 2: U_K -> X_N[0 .. K) and the packed message
// One wave per 256 message bits: the systematic part goes out as it came in, and the packed copy (ceil(K_ldpc / 32) words per frame, zero behind bit
// K: the layout tx_bch_remainder divides) is the 32nd part of it on top.
__global__ void __launch_bounds__(256)
txt_bch_pack_kernel(const int32_t *__restrict__ U, int32_t *__restrict__ X, uint32_t *__restrict__ packed, int K, int N, int vin, int vout)
{
    const int f = blockIdx.y, lane = threadIdx.x & 63;
    const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);                       // wave-uniform
    const int i = 256 * chunk + 4 * lane;
    const txt_i4 b = txt_load4(U + (size_t)f * K, i, K, vin);
    txt_store4(X + (size_t)f * N, i, K, vout, b);
    const uint32_t w = txt_pack256(b, lane);
    const int nw = (K + 31) / 32, wi = 8 * chunk + lane;
    if (lane < 8 && wi < nw) packed[(size_t)f * ((N + 31) / 32) + wi] = w;
}
// ---------------------------------------------------------------- BCH encode, 2 of 2: the parity bits into X_N[K .. N)
__global__ void __launch_bounds__(64)
txt_bchpar_kernel(const TxKParams p, int32_t *X)
{
    __shared__ unsigned long long T[256][3];
    __shared__ uint8_t brev[256];
    const TxBchRem R = tx_bch_remainder(p, T, brev);
    // the 16 lanes of a frame write parity bit j = seg, seg + 16, .. , one int32 per bit, to X[f][K .. K + r) of a socket with K_ldpc elements per frame
    if (!R.live) return;
    const int r = p.K_ldpc - p.K_bch;
    int32_t *o = X + (size_t)R.f * p.K_ldpc + p.K_bch;
    for (int j = R.seg; j < r; j += TX_BCH_SEG) o[j] = (int32_t)tx_bch_parity_bit(R, r, j);
}
hipError_t tx_bch_encode_launch(const TxKParams &p, const int32_t *U, int32_t *X, hipStream_t s)
{
    const int K = p.K_bch, N = p.K_ldpc;
    const int vin = (K & 3) == 0 && txt_al16(U), vout = (K & 3) == 0 && (N & 3) == 0 && txt_al16(X);
    hipLaunchKernelGGL(txt_bch_pack_kernel, dim3((K + 1023) / 1024, p.n_frames), dim3(256), 0, s, U, X, p.bch_cw, K, N, vin, vout);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(txt_bchpar_kernel, dim3((p.n_frames + 64 / TX_BCH_SEG - 1) / (64 / TX_BCH_SEG)), dim3(64), 0, s, p, X);
    return hipGetLastError();
}

// ---------------------------------------------------------------- LDPC encode: one launch, socket in and socket out
// One workgroup (6 waves) per frame, as tx_ldpc_kernel: the waves pack the K_ldpc information bits into LDS 256 at a time, tx_ldpc_rows forms the
// parity rows there, and every lane leaves with four bits of the code word per store -- the information bits back out of LDS (the socket is read
// once), the parity bits p_0 .. p_{M-1} in natural order, p_c at (row c mod q, column c / q) of the rows.
__global__ void __launch_bounds__(LDPC_THREADS)
txt_ldpc_kernel(const TxKParams p, const int32_t *__restrict__ U, int32_t *__restrict__ X, int vin, int vout)
{
    extern __shared__ uint32_t sm[];
    const int K = p.K_ldpc, N = p.N_ldpc, q = (N - K) / LDPC_Z;
    const int nw_in = (K + 31) / 32;
    const TxLdpcLds L = tx_ldpc_lds(sm, p);
    const int t = threadIdx.x, f = blockIdx.x, lane = t & 63;
    for (int w = t; w < q * p.enc_stride; w += LDPC_THREADS) L.tab[w] = p.enc_tab[w];
    if (t == 0) L.info[nw_in] = 0u;
    const int32_t *src = U + (size_t)f * K;
    for (int chunk = t >> 6; chunk < (K + 255) / 256; chunk += LDPC_THREADS / 64) {          // wave-uniform trip count: the ballots see whole waves
        const uint32_t w = txt_pack256(txt_load4(src, 256 * chunk + 4 * lane, K, vin), lane);
        const int wi = 8 * chunk + lane;
        if (lane < 8 && wi < nw_in) L.info[wi] = w;
    }
    __syncthreads();
    tx_ldpc_rows(p, L, t);
    __syncthreads();
    int32_t *dst = X + (size_t)f * N;
    for (int i0 = 4 * t; i0 < N; i0 += 4 * LDPC_THREADS) {
        // parity bit c = i - K sits at (r = c mod q, tt = c / q): stepped, one division per four bits
        int c = i0 >= K ? i0 - K : 0, tt = c / q, r = c - tt * q;
        int bit[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int i = i0 + b;
            if (i < K) bit[b] = (int)((L.info[i >> 5] >> (i & 31)) & 1u);
            else if (i < N) { bit[b] = (int)tx_ldpc_parity_bit(L, r, tt); if (++r == q) { r = 0; tt++; } }
            else bit[b] = 0;
        }
        const txt_i4 v = {bit[0], bit[1], bit[2], bit[3]};
        txt_store4(dst, i0, N, vout, v);
    }
}
hipError_t tx_ldpc_encode_launch(const TxKParams &p, const int32_t *U, int32_t *X, hipStream_t s)
{
    const int vin = (p.K_ldpc & 3) == 0 && txt_al16(U), vout = (p.N_ldpc & 3) == 0 && txt_al16(X);
    hipLaunchKernelGGL(txt_ldpc_kernel, dim3(p.n_frames), dim3(LDPC_THREADS), tx_ldpc_lds_bytes(p), s, p, U, X, vin, vout);
    return hipGetLastError();
}

// ---------------------------------------------------------------- Interleaver::interleave: itl[i] = nat[lut[i]]
// lut[row * cols + j] = col(j) * n_rows + row (column/row interleaver, DVBS2.cpp:451-476; col(j) = j or cols - 1 - j).  A lane writes four consecutive
// bits of the interleaved frame; its four reads fall into the `cols` columns of the natural frame, and over a wave every column is read as one
// contiguous stretch.  One column: a copy, 16 bytes in and out.
__global__ void __launch_bounds__(256)
txt_interleave_kernel(const int32_t *__restrict__ nat, int32_t *__restrict__ itl, int N, int cols, int order, int n_rows, int vin, int vout)
{
    const int f = blockIdx.y;
    const int i0 = 4 * (blockIdx.x * blockDim.x + threadIdx.x);
    if (i0 >= N) return;
    const int32_t *src = nat + (size_t)f * N;
    txt_i4 v;
    if (cols <= 1) v = txt_load4(src, i0, N, vin);
    else {
        // the DVB-S2 column counts divide by a constant (multiply + shift); any other count takes the general division
        int row = cols == 3 ? i0 / 3 : cols == 4 ? i0 / 4 : cols == 5 ? i0 / 5 : cols == 2 ? i0 / 2 : i0 / cols, j = i0 - row * cols;
        int b[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            b[k] = i0 + k < N ? src[(order == DVBS2HIP_ITL_TOP_LEFT ? j : cols - 1 - j) * n_rows + row] & 1 : 0;
            if (++j == cols) { j = 0; row++; }
        }
        v = txt_i4{b[0], b[1], b[2], b[3]};
    }
    txt_store4(itl + (size_t)f * N, i0, N, vout, v);
}
hipError_t tx_interleave_launch(const int32_t *nat, int32_t *itl, int N, int cols, int order, int F, hipStream_t s)
{
    const int n_rows = N / (cols > 1 ? cols : 1);
    const int vin = (N & 3) == 0 && txt_al16(nat), vout = (N & 3) == 0 && txt_al16(itl);
    hipLaunchKernelGGL(txt_interleave_kernel, dim3(((N + 3) / 4 + 255) / 256, F), dim3(256), 0, s, nat, itl, N, cols, order, n_rows, vin, vout);
    return hipGetLastError();
}

// ---------------------------------------------------------------- Modem::modulate: symbol k = constellation point sum_b bits[k bps + b] << b
// A lane makes a pair of symbols (one 16-byte store) from 2 bps consecutive bits.
template <int BPS>
__device__ __forceinline__ int txt_point(const int32_t *__restrict__ bits, int bps)
{
    int idx = 0;
    if (BPS > 0) {
#pragma unroll
        for (int b = 0; b < BPS; b++) idx |= (bits[b] & 1) << b;                // (the loads are issued together)
    } else
        for (int b = 0; b < bps; b++) idx |= (bits[b] & 1) << b;
    return idx;
}
template <int BPS>
__global__ void __launch_bounds__(256)
txt_modulate_kernel(const int32_t *__restrict__ X, float *__restrict__ Y, const float *__restrict__ cstl, int bps, int N, int n_sym, int vout)
{
    __shared__ float cs[64];
    if ((int)threadIdx.x < (2 << bps)) cs[threadIdx.x] = cstl[threadIdx.x];
    __syncthreads();
    const int f = blockIdx.y;
    const int k0 = 2 * (blockIdx.x * blockDim.x + threadIdx.x);
    if (k0 >= n_sym) return;
    const int32_t *src = X + (size_t)f * N + (size_t)k0 * bps;
    float2 *out = reinterpret_cast<float2 *>(Y + (size_t)f * 2 * n_sym) + k0;
    const bool two = k0 + 1 < n_sym;
    const int a = txt_point<BPS>(src, bps), b = two ? txt_point<BPS>(src + bps, bps) : 0;
    const float2 y0 = make_float2(cs[2 * a], cs[2 * a + 1]), y1 = make_float2(cs[2 * b], cs[2 * b + 1]);
    if (two && vout) *reinterpret_cast<float4 *>(out) = make_float4(y0.x, y0.y, y1.x, y1.y);
    else { out[0] = y0; if (two) out[1] = y1; }
}
hipError_t tx_modulate_launch(const int32_t *X, float *Y, const float *cstl, int bps, int N, int n_sym, int F, hipStream_t s)
{
    if (bps < 1 || bps > 5 || (long long)n_sym * bps > N) return hipErrorInvalidValue;      // 64 floats of LDS: at most 32 points; the symbols' bits lie inside the frame
    const dim3 g(((n_sym + 1) / 2 + 255) / 256, F), b(256);
    const int vout = (n_sym & 1) == 0 && txt_al16(Y);
    if (bps == 2) hipLaunchKernelGGL((txt_modulate_kernel<2>), g, b, 0, s, X, Y, cstl, bps, N, n_sym, vout);
    else if (bps == 3) hipLaunchKernelGGL((txt_modulate_kernel<3>), g, b, 0, s, X, Y, cstl, bps, N, n_sym, vout);
    else if (bps == 4) hipLaunchKernelGGL((txt_modulate_kernel<4>), g, b, 0, s, X, Y, cstl, bps, N, n_sym, vout);
    else if (bps == 5) hipLaunchKernelGGL((txt_modulate_kernel<5>), g, b, 0, s, X, Y, cstl, bps, N, n_sym, vout);
    else hipLaunchKernelGGL((txt_modulate_kernel<0>), g, b, 0, s, X, Y, cstl, bps, N, n_sym, vout);
    return hipGetLastError();
}

// ---------------------------------------------------------------- Framer::generate (Framer.hxx:232-293)
// PL frame = 90 header symbols | [16 slots of data | 36 pilots] x n_pil | the remaining data.  A lane writes a pair of PL symbols.  `vec` (the
// launcher: both frame sizes even, both sockets 16-byte aligned): 90, 1440 and 36 are even, so a pair never straddles two kinds and its two data symbols are
// neighbours in the XFEC frame -- one 16-byte load, one 16-byte store.
__device__ __forceinline__ int txt_pl_source(int i, int n_pil, bool &pilot)      // PL symbol i >= 90 -> XFEC symbol (inverse of pl_index, rx_device.h)
{
    const int j = i - PL_M, blk = j / (PL_GAP + PL_P), off = j - blk * (PL_GAP + PL_P);
    pilot = blk < n_pil && off >= PL_GAP;
    return blk < n_pil ? blk * PL_GAP + off : n_pil * PL_GAP + (j - n_pil * (PL_GAP + PL_P));
}
__global__ void __launch_bounds__(256)
txt_framer_kernel(const float *__restrict__ X, float *__restrict__ Y, const float *__restrict__ plh, int n_sym, int pl_frame, int vec)
{
    const int f = blockIdx.y;
    const int i0 = 2 * (blockIdx.x * blockDim.x + threadIdx.x);
    if (i0 >= pl_frame) return;
    const float2 *src = reinterpret_cast<const float2 *>(X + (size_t)f * 2 * n_sym);
    float2 *out = reinterpret_cast<float2 *>(Y + (size_t)f * 2 * pl_frame) + i0;
    const int n_pil = n_sym / PL_GAP;                                               // the count dvbs2hip_create sizes pl_frame with (DVBS2.cpp:351-355): a block follows the last 16 slots too when n_sym is a multiple of 1440
    const float2 pil = make_float2(0.70710678118654752440f, 0.70710678118654752440f);     // Framer.hxx:252-260
    if (vec) {
        float4 y;
        bool pilot = false;
        if (i0 < PL_M) y = *reinterpret_cast<const float4 *>(plh + 2 * i0);
        else {
            const int k = txt_pl_source(i0, n_pil, pilot);
            y = pilot ? make_float4(pil.x, pil.y, pil.x, pil.y) : *reinterpret_cast<const float4 *>(src + k);
        }
        *reinterpret_cast<float4 *>(out) = y;
        return;
    }
    for (int u = 0; u < 2 && i0 + u < pl_frame; u++) {
        const int i = i0 + u;
        float2 y;
        if (i < PL_M) y = make_float2(plh[2 * i], plh[2 * i + 1]);
        else {
            bool pilot;
            const int k = txt_pl_source(i, n_pil, pilot);
            y = pilot ? pil : src[k];
        }
        out[u] = y;
    }
}
hipError_t tx_framer_launch(const float *X, float *Y, const float *plh, int n_sym, int pl_frame, int F, hipStream_t s)
{
    const int vec = (n_sym & 1) == 0 && (pl_frame & 1) == 0 && txt_al16(X) && txt_al16(Y) && txt_al16(plh);
    hipLaunchKernelGGL(txt_framer_kernel, dim3(((pl_frame + 1) / 2 + 255) / 256, F), dim3(256), 0, s, X, Y, plh, n_sym, pl_frame, vec);
    return hipGetLastError();
}

// ---------------------------------------------------------------- Scrambler_PL::scramble (Scrambler_PL.hxx:61-78, scr_flag = true)
// multiply by exp(j pi/2 R): R = 1: (-y, x), 2: (-x, -y), 3: (y, -x) -- a swap and sign flips; the 90 header symbols are copied
__device__ __forceinline__ float2 txt_rotate(float2 y, int R)
{
    const float a = (R & 1) ? -y.y : y.x, b = (R & 1) ? y.x : y.y;
    return (R & 2) ? make_float2(-a, -b) : make_float2(a, b);
}
__global__ void __launch_bounds__(256)
txt_pl_scramble_kernel(const float *__restrict__ X, float *__restrict__ Y, const uint8_t *__restrict__ seq, int pl_frame, int vec)
{
    const int f = blockIdx.y;
    const int i0 = 2 * (blockIdx.x * blockDim.x + threadIdx.x);
    if (i0 >= pl_frame) return;
    const float2 *src = reinterpret_cast<const float2 *>(X + (size_t)f * 2 * pl_frame) + i0;
    float2 *out = reinterpret_cast<float2 *>(Y + (size_t)f * 2 * pl_frame) + i0;
    if (vec) {                                                                      // pl_frame is even: the pair is whole
        const float4 v = *reinterpret_cast<const float4 *>(src);
        float2 y0 = make_float2(v.x, v.y), y1 = make_float2(v.z, v.w);
        if (i0 >= PL_M) { y0 = txt_rotate(y0, seq[i0 - PL_M] & 3); y1 = txt_rotate(y1, seq[i0 + 1 - PL_M] & 3); }       // (90 is even: header or data, both)
        *reinterpret_cast<float4 *>(out) = make_float4(y0.x, y0.y, y1.x, y1.y);
        return;
    }
    for (int u = 0; u < 2 && i0 + u < pl_frame; u++) {
        const int i = i0 + u;
        float2 y = src[u];
        if (i >= PL_M) y = txt_rotate(y, seq[i - PL_M] & 3);
        out[u] = y;
    }
}
hipError_t tx_pl_scramble_launch(const float *X, float *Y, const uint8_t *seq, int pl_frame, int F, hipStream_t s)
{
    const int vec = (pl_frame & 1) == 0 && txt_al16(X) && txt_al16(Y);
    hipLaunchKernelGGL(txt_pl_scramble_kernel, dim3(((pl_frame + 1) / 2 + 255) / 256, F), dim3(256), 0, s, X, Y, seq, pl_frame, vec);
    return hipGetLastError();
}

}  // namespace dvbs2
