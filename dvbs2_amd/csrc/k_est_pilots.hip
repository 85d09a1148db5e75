// Pilot-aided noise estimator: sigma, Eb/N0 and Es/N0 of an aligned PL frame from the symbols the receiver knows -- the 90 header symbols and the 36 symbols of every
// pilot block.  An extension: the reference's only estimator is Estimator_DVBS2 (M2M4, estimate_kernel of k_front.hip), whose Se = sqrt(|2 m2^2 - m4|) takes every
// constellation point to have the same modulus and so reads 16APSK and 32APSK several dB low; a data-aided estimate does not care what the data symbols are.
//
// The definition (include/dvbs2hip.h; float64 twin: tests/est_pilots_ref.py).  Known position k of L = 90 + 36 N_pilots: k < 90 is frame position k and carries the
// handle's PLHEADER (plheader() of api_tables.hip), k = 90 + 36 b + i is frame position k + 1440 (b + 1) and carries (1 + j) / sqrt(2).  With y[k] the received and
// p[k] the known value (scrambled = 1: the pilots first PL-descrambled, the swap / sign change of pl_descramble_kernel, exact):
//   c = (1/L) sum_k y[k] conj(p[k])      N = sum_k |y[k] - c p[k]|^2 / (L - 1)      A = |c|^2      S = A - N / L      Es_N0 = 10 log10(S / N)
// the residual form: no small number is the difference of two large ones.  S <= 0: -100 dB; N = 0, or a ratio above 100 dB: +100 dB (an fp32 frame without noise
// leaves N near 1e-14 A, not 0).  SIG and Eb_N0 from Es_N0 as the M2M4 estimator forms them (esn0_to_sigma_ebn0, rx_device.h).
// The estimate is coherent over the frame: a constant phase does not move it, a residual carrier lowers S -- it belongs behind the fine synchronizers, or on a baseband
// loop without a carrier error; removing the carrier is not this task's job.
//
// One wave per frame, four per workgroup, no LDS, no scratch.  Lane l holds the known symbols l, l + 64, .. (NJ = ceil(L / 64) <= 14 of them, 8-byte loads: a located
// frame is 8-byte aligned and no more) in registers across both passes; the two sums are a serial sum per lane, then an all-reduce in six xor steps (DPP, swizzle, one
// bpermute), so every lane ends with the same c and N.  fp32 in this order: bit-exact with nothing, held to float64 by tests/test_est_pilots_gpu.py.
// alpha > 0 (averaging over a stream's frames): the launch leaves (A, N) per frame, est_pilots_walk_kernel takes each stream's frames in order, one lane per stream.
#include "dvbs2hip_internal.h"
#include "rx_device.h"

namespace dvbs2 {

constexpr int ESTP_WAVES = 4;                    // frames (= waves) per workgroup; the waves never meet

namespace {

// (A, N) -> the three outputs
__device__ __forceinline__ void estp_finish(float A, float N, float rL, float rate_bps, float &sigma, float &ebn0, float &esn0)
{
    const float S = A - N * rL;
    esn0 = 10.f * 0.301029995663981f * __builtin_amdgcn_logf(S * __builtin_amdgcn_rcpf(N));       // 10 log10(S / N)
    if (!(S > 0.f)) esn0 = -100.f;
    else if (N == 0.f || !(esn0 < 100.f)) esn0 = 100.f;
    esn0_to_sigma_ebn0(esn0, rate_bps, sigma, ebn0);
}

}  // namespace

struct EstpKParams {
    const float2 *x; const float2 *const *src; size_t stride;      // frame f at x + f stride (float2 units) or at src[f], 8-byte aligned and no more
    const float2 *plh; const uint8_t *seq;                          // the handle's PLHEADER (90) and PL sequence R(i) (position i + 90)
    float *AN, *SIG, *EB, *ES;                                      // AN: [F][2], the averaging form's (A, N), and then no outputs from this launch
    float rL, rL1, rate_bps;
    int32_t L, compact, scrambled, F;                               // compact: the frame holds its L known symbols and nothing else (the host form's staging)
};

template <int NJ>
__global__ void __launch_bounds__(64 * ESTP_WAVES)
est_pilots_kernel(const EstpKParams p)
{
    const int f = blockIdx.x * ESTP_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (one value per wave: the frame's address is a scalar)
    if (f >= p.F) return;
    const int lane = threadIdx.x & 63;
    const float2 *r = p.src ? p.src[f] : p.x + (size_t)f * p.stride;
    const float a = 0.70710678118654752f;
    float2 y[NJ], ph[2];                           // the lane's symbols; the known values of the first two (a header symbol only there: 90 < 128)
    float cr = 0.f, ci = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int k = lane + 64 * j;
        const bool valid = k < p.L;
        const int kk = valid ? k : 0;
        const bool pil = kk >= PL_M;
        const int pos = pl_known_index(kk);
        float2 v = r[p.compact ? kk : pos];
        const int R = pil && p.scrambled ? (int)p.seq[pos - PL_M] : 0;
        v = pl_derotate(v, R);
        float2 q = make_float2(a, a);
        if (j < 2) { if (!pil) q = p.plh[kk]; }
        if (!valid) { v = make_float2(0.f, 0.f); q = v; }
        y[j] = v;
        if (j < 2) ph[j] = q;
        cr += v.x * q.x + v.y * q.y;
        ci += v.y * q.x - v.x * q.y;
    }
    cr = wave_sum(cr) * p.rL; ci = wave_sum(ci) * p.rL;
    float n = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const float w = lane + 64 * j < p.L ? a : 0.f;
        const float2 q = j < 2 ? ph[j] : make_float2(w, w);
        const float er = y[j].x - (cr * q.x - ci * q.y), ei = y[j].y - (cr * q.y + ci * q.x);
        n += er * er + ei * ei;
    }
    const float N = wave_sum(n) * p.rL1, A = cr * cr + ci * ci;
    if (lane != 0) return;
    if (p.AN) { p.AN[2 * f] = A; p.AN[2 * f + 1] = N; return; }
    float sigma, ebn0, esn0;
    estp_finish(A, N, p.rL, p.rate_bps, sigma, ebn0, esn0);
    if (p.SIG) p.SIG[f] = sigma;
    if (p.EB) p.EB[f] = ebn0;
    if (p.ES) p.ES[f] = esn0;
}

// stream s = frames [s Fs, (s + 1) Fs), in order; st: {Abar, Nbar, started} per stream
__global__ void __launch_bounds__(64)
est_pilots_walk_kernel(const float *__restrict__ AN, float *__restrict__ st, float alpha, float rL, float rate_bps, float *__restrict__ SIG, float *__restrict__ EB,
                       float *__restrict__ ES, int Fs, int S)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    float Ab = st[3 * s], Nb = st[3 * s + 1];
    bool started = st[3 * s + 2] != 0.f;
    const float beta = 1.f - alpha;
    for (int f = s * Fs; f < (s + 1) * Fs; f++) {
        const float A = AN[2 * f], N = AN[2 * f + 1];
        if (started) { Ab = alpha * Ab + beta * A; Nb = alpha * Nb + beta * N; }
        else { Ab = A; Nb = N; started = true; }
        float sigma, ebn0, esn0;
        estp_finish(Ab, Nb, rL, rate_bps, sigma, ebn0, esn0);
        if (SIG) SIG[f] = sigma;
        if (EB) EB[f] = ebn0;
        if (ES) ES[f] = esn0;
    }
    st[3 * s] = Ab; st[3 * s + 1] = Nb; st[3 * s + 2] = 1.f;
}

hipError_t est_pilots_launch(const float *X, const float *const *SRC, size_t stride_cplx, int compact, const float *plh, const uint8_t *seq, int scrambled, int L,
                             float code_rate, int bps, float *AN, float *SIG, float *EB, float *ES, int F, hipStream_t s)
{
    EstpKParams p;
    p.x = reinterpret_cast<const float2 *>(X); p.src = reinterpret_cast<const float2 *const *>(SRC); p.stride = stride_cplx;
    p.plh = reinterpret_cast<const float2 *>(plh); p.seq = seq; p.AN = AN; p.SIG = SIG; p.EB = EB; p.ES = ES;
    p.rL = 1.f / (float)L; p.rL1 = 1.f / (float)(L - 1); p.rate_bps = code_rate * (float)bps;
    p.L = L; p.compact = compact; p.scrambled = scrambled; p.F = F;
    const dim3 g((unsigned)((F + ESTP_WAVES - 1) / ESTP_WAVES)), b(64 * ESTP_WAVES);
    switch ((L + 63) / 64) {
#define ESTP_CASE(n) case n: hipLaunchKernelGGL(est_pilots_kernel<n>, g, b, 0, s, p); break;
        ESTP_CASE(2) ESTP_CASE(3) ESTP_CASE(4) ESTP_CASE(5) ESTP_CASE(6) ESTP_CASE(7) ESTP_CASE(8) ESTP_CASE(9) ESTP_CASE(10) ESTP_CASE(11) ESTP_CASE(12) ESTP_CASE(13) ESTP_CASE(14)
#undef ESTP_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t est_pilots_walk_launch(const float *AN, float *state, float alpha, int L, float code_rate, int bps, float *SIG, float *EB, float *ES, int Fs, int S, hipStream_t s)
{
    hipLaunchKernelGGL(est_pilots_walk_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, s, AN, state, alpha, 1.f / (float)L, code_rate * (float)bps, SIG, EB, ES, Fs, S);
    return hipGetLastError();
}

}  // namespace dvbs2
