// PLS decoder: which of the 256 PLHEADERs the transmitter's framer can build (Framer.hxx:97-196 of the reference, plheader() of api_tables.hip) an aligned PL frame
// starts with.  An extension: the reference fixes the MODCOD on the command line and has no task that reads the field.
//
// The value: V = b0 128 + b1 64 + ... + b6 2 + p, with b0..b6 the seven bits that multiply the rows of G (row 0 the extension row, rows 1-5 the Walsh rows with row 1
// alternating fastest, row 6 all ones) and p the pairing of the 64 coded bits, y[2i] = c[i], y[2i+1] = c[i] ^ p (the framer always sends p = 1).
// The metric of a hypothesis H (90 unit symbols: the SOF, then the scrambled pi/2-BPSK code word, times j when b0 = 1): |sum_k r[k] conj(H[k])| = |S + P|, S over the
// 26 SOF symbols, P over the 64 PLS symbols -- maximum likelihood for an unknown constant phase, the SOF telling a code word from its complement.  The largest metric
// wins, the smallest V among equal ones.
//
// One wave per frame, no LDS, no scratch:
//   1. lane k loads PLS symbol k (lanes 0-25 the SOF symbol k too) and takes the pi/2 rotation and the scrambler's sign off it -- times sqrt(2): a multiplication by
//      (1 - j) or (-1 - j) is two additions, and the factor leaves with the one multiplication by 1/2 under the square root;
//   2. the pairs: even lane 2i forms d[2i] + d[2i+1] (p = 0), odd lane 2i+1 forms d[2i] - d[2i+1] (p = 1); one permute then puts z_p[i] into lane 32 p + i, so the two
//      halves of the wave carry the two pairing hypotheses;
//   3. b0 = 1 is a second value per lane: z times -j times the sign of row 0;
//   4. five butterfly stages inside each half (xor 1, 2, 8: DPP; xor 4, 16: swizzle) leave h_b0[w] = sum_i (-1)^popcount(w & i) z[i] in lane 32 p + w, w = b1 + 2 b2 + .. + 16 b5;
//   5. row 6 is the sign of the whole word: |S + h|^2 and |S - h|^2, for both b0 -- four hypotheses per lane, 256 per wave;
//   6. arg max over the wave on the squared value, one square root.
// fp32, every sum a tree of its own order: the result is held to float64 by tests/test_pls_gpu.py, bit-exact with nothing.
#include "dvbs2hip_internal.h"
#include "rx_device.h"

namespace dvbs2 {

constexpr int PLS_WAVES = 4;                     // frames (= waves) per workgroup; the waves never meet

namespace {

constexpr int PLS_G0[32] = {1,0,0,1,0,0,0,0,1,0,1,0,1,1,0,0,0,0,1,0,1,1,0,1,1,1,0,1,1,1,0,1};      // row 0 of G, Framer.hxx:103-104
constexpr int PLS_SCR[64] = {0,1,1,1,0,0,0,1,1,0,0,1,1,1,0,1,1,0,0,0,0,0,1,1,1,1,0,0,1,0,0,1,0,1,0,1,0,0,1,1,0,1,0,0,0,0,1,0,0,0,1,0,1,1,0,1,1,1,1,1,1,0,1,0};
constexpr int PLS_SOF[26] = {0,1,1,0,0,0,1,1,0,1,0,0,1,0,1,1,1,0,1,0,0,0,0,0,1,0};
template <int N> constexpr unsigned long long pls_mask(const int (&b)[N]) { unsigned long long m = 0; for (int i = 0; i < N; i++) m |= (unsigned long long)(b[i] & 1) << i; return m; }
constexpr unsigned long long PLS_SCR_M = pls_mask(PLS_SCR);
constexpr uint32_t PLS_SOF_M = (uint32_t)pls_mask(PLS_SOF), PLS_G0_M = (uint32_t)pls_mask(PLS_G0);

// (wave_xor<M>, the value of lane l ^ M: rx_device.h)
template <int M> __device__ __forceinline__ void pls_sum3(float &a, float &b, float &c) { a = a + wave_xor<M>(a); b = b + wave_xor<M>(b); c = c + wave_xor<M>(c); }
// one stage of the Hadamard transform on the lane's two complex values: the lane without bit M takes own + other, the lane with it other - own
template <int M> __device__ __forceinline__ void pls_bfly(float (&u)[4], int lane)
{
    const bool hi = lane & M;
#pragma unroll
    for (int c = 0; c < 4; c++) { const float o = wave_xor<M>(u[c]); u[c] = o + (hi ? -u[c] : u[c]); }
}
// the larger squared metric, the smaller value among equal ones
template <int M> __device__ __forceinline__ void pls_max(float &m2, uint32_t &v)
{
    const float om = wave_xor<M>(m2); const uint32_t ov = wave_xor<M>(v);
    if (om > m2 || (om == m2 && ov < v)) { m2 = om; v = ov; }
}

}  // namespace

// x + f * stride (float2 units) or src[f]: the start of frame f, 8-byte aligned and no more
__global__ void __launch_bounds__(64 * PLS_WAVES)
pls_decode_kernel(const float2 *__restrict__ x, const float2 *const *__restrict__ src, size_t stride, int32_t *__restrict__ PLS, float *__restrict__ MET, float *__restrict__ ENE, int F)
{
    const int f = blockIdx.x * PLS_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (one value per wave: the frame's address is a scalar)
    if (f >= F) return;
    const int lane = threadIdx.x & 63;
    const float2 *r = src ? src[f] : x + (size_t)f * stride;
    const float2 q = r[26 + lane];
    const float2 s = lane < 26 ? r[lane] : make_float2(0.f, 0.f);
    float ene = (q.x * q.x + q.y * q.y) + (s.x * s.x + s.y * s.y);
    // times conj of sqrt(2) times the symbol of bit 0: (1 - j) at an even position, (-1 - j) at an odd one; then the sign of the known bit
    const bool odd = lane & 1;
    const float ssg = (PLS_SOF_M >> (lane & 31)) & 1u ? -1.f : 1.f;                // (lanes >= 26 hold zeros)
    float sre = ssg * (odd ? s.y - s.x : s.x + s.y), sim = ssg * (odd ? -s.x - s.y : s.y - s.x);
    pls_sum3<1>(sre, sim, ene); pls_sum3<2>(sre, sim, ene); pls_sum3<4>(sre, sim, ene); pls_sum3<8>(sre, sim, ene); pls_sum3<16>(sre, sim, ene); pls_sum3<32>(sre, sim, ene);
    const float dsg = (PLS_SCR_M >> lane) & 1ull ? -1.f : 1.f;
    const float dre = dsg * (odd ? q.y - q.x : q.x + q.y), dim = dsg * (odd ? -q.x - q.y : q.y - q.x);
    // even lane 2i: d[2i] + d[2i+1]; odd lane 2i+1: d[2i] - d[2i+1]
    float zre = wave_xor<1>(dre) + (odd ? -dre : dre), zim = wave_xor<1>(dim) + (odd ? -dim : dim);
    // lane 32 p + i takes z_p[i] from lane 2 i + p
    const int from = ((lane & 31) << 1 | lane >> 5) << 2;
    zre = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(from, __builtin_bit_cast(int, zre)));
    zim = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(from, __builtin_bit_cast(int, zim)));
    // b0 = 1: the symbols were multiplied by j and row 0 was added to the word
    const float g0 = (PLS_G0_M >> (lane & 31)) & 1u ? -1.f : 1.f;
    float u[4] = {zre, zim, g0 * zim, -(g0 * zre)};
    pls_bfly<1>(u, lane); pls_bfly<2>(u, lane); pls_bfly<4>(u, lane); pls_bfly<8>(u, lane); pls_bfly<16>(u, lane);
    // lane 32 p + w, w = b1 + 2 b2 + 4 b3 + 8 b4 + 16 b5: the four hypotheses (b0, b6) in the order of their values
    const uint32_t w = lane & 31;
    const uint32_t v0 = (__brev(w) >> 27) << 2 | (uint32_t)lane >> 5;
    float m2 = -1.f; uint32_t v = 0;
#pragma unroll
    for (int b0 = 0; b0 < 2; b0++)
#pragma unroll
        for (int b6 = 0; b6 < 2; b6++) {
            const float tr = b6 ? sre - u[2 * b0] : sre + u[2 * b0], ti = b6 ? sim - u[2 * b0 + 1] : sim + u[2 * b0 + 1];
            const float t2 = tr * tr + ti * ti;
            if (t2 > m2) { m2 = t2; v = v0 | (uint32_t)b0 << 7 | (uint32_t)b6 << 1; }
        }
    pls_max<1>(m2, v); pls_max<2>(m2, v); pls_max<4>(m2, v); pls_max<8>(m2, v); pls_max<16>(m2, v); pls_max<32>(m2, v);
    if (lane == 0) {
        PLS[f] = (int32_t)v;
        if (MET) MET[f] = sqrtf(0.5f * m2);
        if (ENE) ENE[f] = ene;
    }
}

hipError_t pls_decode_launch(const float *X, const float *const *SRC, size_t stride_cplx, int32_t *PLS, float *MET, float *ENE, int F, hipStream_t s)
{
    hipLaunchKernelGGL(pls_decode_kernel, dim3((unsigned)((F + PLS_WAVES - 1) / PLS_WAVES)), dim3(64 * PLS_WAVES), 0, s, reinterpret_cast<const float2 *>(X),
                       reinterpret_cast<const float2 *const *>(SRC), stride_cplx, PLS, MET, ENE, F);
    return hipGetLastError();
}

}  // namespace dvbs2
