// PLHEADER search: the PLS decoder (k_pls.hip) at every symbol offset of a buffer, and the offset and value whose headers repeat at the frame length the value implies
// (include/dvbs2hip.h has the definition).  An extension with no reference task.
//
// Scan.  Output k is what pls_decode_kernel returns for a frame that starts at symbol k, bit for bit: every sum of that kernel is a fixed tree and fp32 addition is
// commutative, so the same trees are built here in another place.  That kernel spends a wave per frame and most of its instructions on cross-lane moves; here the lanes
// lie across offsets -- lane l of a workgroup works on offset 64 blockIdx.x + l -- so position k of the header is the same for every lane, and the pi/2 rotation, the
// scrambler's sign, the SOF's sign and row 0's sign are compile-time choices between add and subtract.  No DPP, swizzle or permute.
//   - 256 threads stage the workgroup's 64 + 89 symbols and their |x|^2 in LDS (zeros past the buffer's end: no lane reads global memory after that);
//   - the four waves take the four (pairing p, b0) hypotheses: each forms the SOF sum (the tree of the 64-lane xor all-reduce with zeros past lane 25), the pair sums
//     z_p[i], its 32-point transform in its own registers (five stages, `other + (+-own)`), and the 64 hypotheses (w, b6) in the order of their values, strict >;
//   - wave 0 also forms the energy (the same all-reduce tree), then merges the four (m2, v) through LDS -- larger m2, then smaller v -- and writes PLS, MET, ENE.
// The waves of a workgroup meet at two barriers; no workgroup waits on another.  No scratch.
//
// Search.  One lane per offset walks its chain of slots k, k + L, .. serially (a buffer of a few frames gives a handful) and the workgroup keeps its best (C, then smaller
// k); a second launch of one workgroup reduces the workgroups' bests and writes RES and SCORE.
#include "dvbs2hip_internal.h"

namespace dvbs2 {

namespace {

constexpr int PSS_G0[32] = {1,0,0,1,0,0,0,0,1,0,1,0,1,1,0,0,0,0,1,0,1,1,0,1,1,1,0,1,1,1,0,1};      // row 0 of G, Framer.hxx:103-104
constexpr int PSS_SCR[64] = {0,1,1,1,0,0,0,1,1,0,0,1,1,1,0,1,1,0,0,0,0,0,1,1,1,1,0,0,1,0,0,1,0,1,0,1,0,0,1,1,0,1,0,0,0,0,1,0,0,0,1,0,1,1,0,1,1,1,1,1,1,0,1,0};
constexpr int PSS_SOF[26] = {0,1,1,0,0,0,1,1,0,1,0,0,1,0,1,1,1,0,1,0,0,0,0,0,1,0};
constexpr int pss_brev5(int w) { return (w & 1) << 4 | (w & 2) << 2 | (w & 4) | (w & 8) >> 2 | (w & 16) >> 4; }

constexpr int PSS_OFFS = 64;                     // offsets per workgroup: one per lane, the four waves share them
constexpr int PSS_SYMS = PSS_OFFS + 89;          // symbols a workgroup reads

// a[0] = the sum of a[0 .. N) in the order of the xor all-reduce: neighbours first
template <int N> __device__ __forceinline__ void pss_tree(float (&a)[N])
{
#pragma unroll
    for (int step = 1; step < N; step *= 2)
#pragma unroll
        for (int i = 0; i < N; i += 2 * step) a[i] = a[i] + a[i + step];
}

// hypotheses (p, b0) of the offset whose header starts at r[0]: the largest |S + P|^2 of its 64 values and the smallest value that reaches it
template <int P, int B0>
__device__ __forceinline__ void pss_pass(const float2 *r, float &m2, uint32_t &v)
{
    // S: times conj of sqrt(2) times the symbol of bit 0 -- (1 - j) at an even position, (-1 - j) at an odd one -- then the SOF's sign; zeros past 25.  The top of the
    // 64-lane tree adds a zero to this sum and is left out (a zero's sign never reaches a result: every t2 is a sum of squares)
    float sr[32], si[32];
#pragma unroll
    for (int k = 0; k < 32; k++) {
        if (k < 26) {
            const float2 s = r[k];
            const float re = k & 1 ? s.y - s.x : s.x + s.y, im = k & 1 ? -s.x - s.y : s.y - s.x;
            sr[k] = PSS_SOF[k] ? -re : re; si[k] = PSS_SOF[k] ? -im : im;
        } else sr[k] = si[k] = 0.f;
    }
    pss_tree(sr); pss_tree(si);
    const float sre = sr[0], sim = si[0];
    // z_p[i] from d[2i] (even position) and d[2i+1] (odd position), then the b0 = 1 form: times -j times the sign of row 0
    float ur[32], ui[32];
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const float2 a = r[26 + 2 * i], b = r[27 + 2 * i];
        float are = a.x + a.y, aim = a.y - a.x, bre = b.y - b.x, bim = -b.x - b.y;
        if (PSS_SCR[2 * i]) { are = -are; aim = -aim; }
        if (PSS_SCR[2 * i + 1]) { bre = -bre; bim = -bim; }
        const float zre = P ? are + (-bre) : bre + are, zim = P ? aim + (-bim) : bim + aim;
        if (B0) { ur[i] = PSS_G0[i] ? -zim : zim; ui[i] = PSS_G0[i] ? zre : -zre; }
        else { ur[i] = zre; ui[i] = zim; }
    }
    // the index without bit M takes other + own, the index with it other - own
#pragma unroll
    for (int M = 1; M < 32; M *= 2)
#pragma unroll
        for (int i = 0; i < 32; i++)
            if (!(i & M)) {
                const float ar = ur[i], br = ur[i | M], ai = ui[i], bi = ui[i | M];
                ur[i] = br + ar; ur[i | M] = ar + (-br);
                ui[i] = bi + ai; ui[i | M] = ai + (-bi);
            }
    // w = b1 + 2 b2 + .. + 16 b5: in the order of the values, so that strict > keeps the smallest among equal ones
    m2 = -1.f; v = 0;
#pragma unroll
    for (int c = 0; c < 32; c++) {
        const int w = pss_brev5(c);
#pragma unroll
        for (int b6 = 0; b6 < 2; b6++) {
            const float tr = b6 ? sre - ur[w] : sre + ur[w], ti = b6 ? sim - ui[w] : sim + ui[w];
            const float t2 = tr * tr + ti * ti;
            if (t2 > m2) { m2 = t2; v = (uint32_t)(B0 << 7 | c << 2 | b6 << 1 | P); }
        }
    }
}

struct PssBest { float c; int32_t k, count, slots; };
__device__ __forceinline__ bool pss_better(const PssBest &a, const PssBest &b) { return a.c > b.c || (a.c == b.c && a.k < b.k); }

// the best of the workgroup's 256 entries, in thread 0
__device__ __forceinline__ PssBest pss_block_best(PssBest b, PssBest *sm)
{
    sm[threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && pss_better(sm[threadIdx.x + s], sm[threadIdx.x])) sm[threadIdx.x] = sm[threadIdx.x + s];
        __syncthreads();
    }
    return sm[0];
}

}  // namespace

__global__ void __launch_bounds__(256)
pls_scan_kernel(const float2 *__restrict__ x, int n_sym, int32_t *__restrict__ PLS, float *__restrict__ MET, float *__restrict__ ENE, int K)
{
    __shared__ float2 sx[PSS_SYMS + 3];
    __shared__ float se[PSS_SYMS + 3];
    __shared__ float sm2[3][64];
    __shared__ uint32_t sv[3][64];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long o0 = (long long)blockIdx.x * PSS_OFFS;
    if (t < PSS_SYMS) {
        const long long i = o0 + t;
        const float2 q = i < n_sym ? x[i] : make_float2(0.f, 0.f);
        sx[t] = q; se[t] = q.x * q.x + q.y * q.y;
    }
    __syncthreads();
    const float2 *r = sx + lane;
    float m2; uint32_t v;
    if (wave == 0) pss_pass<0, 0>(r, m2, v);
    else if (wave == 1) pss_pass<1, 0>(r, m2, v);
    else if (wave == 2) pss_pass<0, 1>(r, m2, v);
    else pss_pass<1, 1>(r, m2, v);
    float ene = 0.f;
    if (wave == 0) {
        float e[64];
#pragma unroll
        for (int l = 0; l < 64; l++) e[l] = se[lane + 26 + l] + (l < 26 ? se[lane + l] : 0.f);
        pss_tree(e);
        ene = e[0];
    } else { sm2[wave - 1][lane] = m2; sv[wave - 1][lane] = v; }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 0; w < 3; w++) {
        const float om = sm2[w][lane]; const uint32_t ov = sv[w][lane];
        if (om > m2 || (om == m2 && ov < v)) { m2 = om; v = ov; }
    }
    const long long o = o0 + lane;
    if (o < K) {
        PLS[o] = (int32_t)v;
        if (MET) MET[o] = sqrtf(0.5f * m2);
        if (ENE) ENE[o] = ene;
    }
}

// the chain of every start, and the workgroup's best
__global__ void __launch_bounds__(256)
pls_chain_kernel(const int32_t *__restrict__ PLS, const float *__restrict__ MET, const float *__restrict__ ENE, const int32_t *__restrict__ LEN, PssBest *__restrict__ blk, int K)
{
    __shared__ PssBest sm[256];
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    PssBest b = {-1.f, -1, 0, 0};
    if (k < K) {
        const int32_t v = PLS[k];
        const int32_t L = LEN[v & 255];
        if (L >= 90 && k < L) {
            float C = 0.f; int32_t cnt = 0, J = 0;
            for (long long kj = k; kj < K; kj += L, J++) {
                float q = 0.f;
                if (PLS[kj] == v) {
                    const float m = MET[kj], e = ENE[kj];
                    q = e == 0.f ? 0.f : (m * m) / (90.f * e);
                    cnt++;
                }
                C = C + q;
            }
            b = {C, (int32_t)k, cnt, J};
        }
    }
    b = pss_block_best(b, sm);
    if (threadIdx.x == 0) blk[blockIdx.x] = b;
}

__global__ void __launch_bounds__(256)
pls_pick_kernel(const PssBest *__restrict__ blk, int n_blk, const int32_t *__restrict__ PLS, int32_t *__restrict__ RES, float *__restrict__ SCORE)
{
    __shared__ PssBest sm[256];
    PssBest b = {-1.f, -1, 0, 0};
    for (int i = threadIdx.x; i < n_blk; i += 256) { const PssBest o = blk[i]; if (pss_better(o, b)) b = o; }
    b = pss_block_best(b, sm);
    if (threadIdx.x == 0) {
        const bool found = b.k >= 0;
        RES[0] = found ? b.k : -1; RES[1] = found ? PLS[b.k] : 0; RES[2] = found ? b.count : 0; RES[3] = found ? b.slots : 0;
        *SCORE = found ? b.c : 0.f;
    }
}

hipError_t pls_scan_launch(const float *X, int n_sym, int32_t *PLS, float *MET, float *ENE, hipStream_t s)
{
    const int K = n_sym - 89;
    hipLaunchKernelGGL(pls_scan_kernel, dim3((unsigned)((K + PSS_OFFS - 1) / PSS_OFFS)), dim3(256), 0, s, reinterpret_cast<const float2 *>(X), n_sym, PLS, MET, ENE, K);
    return hipGetLastError();
}

size_t pls_search_work_bytes(int n_sym) { return sizeof(PssBest) * (size_t)((n_sym - 89 + 255) / 256); }

hipError_t pls_search_launch(const int32_t *PLS, const float *MET, const float *ENE, const int32_t *LEN, void *work, int n_sym, int32_t *RES, float *SCORE, hipStream_t s)
{
    const int K = n_sym - 89, n_blk = (K + 255) / 256;
    hipLaunchKernelGGL(pls_chain_kernel, dim3((unsigned)n_blk), dim3(256), 0, s, PLS, MET, ENE, LEN, (PssBest *)work, K);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pls_pick_kernel, dim3(1), dim3(256), 0, s, (const PssBest *)work, n_blk, PLS, RES, SCORE);
    return hipGetLastError();
}

}  // namespace dvbs2
