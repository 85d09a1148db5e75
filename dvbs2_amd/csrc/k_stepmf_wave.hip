// The coarse-frequency loop, one wave per stream: the loop of k_stepmf.hip (its header states the reference's four steps per sample and the arithmetic contract) with
// rotation and matched filter taken out of the serial chain.
//
// nu changes only inside the PLL update, that is only on a strobe at a pilot position (curr_idx >= 1530, curr_idx % 1476 in [54, 90)), and there only when
// floor(-estimated_freq 1e6) changes.  Between two such changes steps 1 and 2 are a feed-forward of the input: the rotation phase of sample n is the integer
// nco_turn_index(nu_k, n), the filter output a fixed-order sum over 81 rotated samples.  So, per stream, until the call's Fs N samples are done:
//   CHUNK  the next c = min(64, samples left) samples behind the last final one
//   AHEAD  lane i < c rotates x_i by nco_turn_index(nu_k, (n + i) mod 1e6) -- the lane form's products and sums --, the z go to LDS behind the 80 samples of history, and
//          lane i sums the matched filter over z[i - 80 .. i] (smf_filter below: the lane form's expression and order)
//   LOOP   i = 0 .. c - 1, the whole wave alike: steps 3 and 4 of k_stepmf.hip as they stand -- frame start, Farrow, gardner_step, Y and B, on a strobe the PLL update and
//          curr_idx, at the frame's end MU / FRQ / PHS -- on lane i's filter output
//   CUT    if the PLL update at sample i changed nu_k, samples 0 .. i are final and the chunk ends there: n and the window advance by i + 1, and the samples behind are
//          rotated again, from the raw input, with the new nu_k in the next chunk.  Otherwise all c are final.
// Nothing is re-associated: every lane evaluates the expression the one lane of stepmf_kernel evaluates, so the results are that kernel's and tests/stepmf_twin.c's bit for
// bit (tests/stepmf_wave_twin.c is this order on the CPU).  State in and out is the lane form's -- StmState, SfcState, the 80 rotated samples oldest first, ccnt -- so a
// handle may change form between any two calls.
//
// The raw samples of a chunk stay in a register per lane; LDS holds rotated samples only ([80 history | 64 chunk] float2 = 1152 B), and a chunk behind a cut loads its raw
// samples from X again.  Y and B are stored once per chunk, lanes across samples, and only the final part of a cut chunk: X is never read at a sample whose Y has been
// written, which is the lane form's rule for the sockets (a tile is read before its outputs are stored).  The next chunk's samples are requested before the serial loop.
#include "gardner_loop.h"
#include "nco_turn.h"

namespace dvbs2 {

constexpr int SMW_H = 80;                          // the matched filter's memory: taps - 1
constexpr int SMW_C = 64;                          // samples per chunk: one per lane

// the value lane `l` holds, for the whole wave (l the same in every lane)
__device__ __forceinline__ float smw_lane(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), __builtin_amdgcn_readfirstlane(l)));
}

// The matched filter over w[0] (oldest) .. w[80] (newest, handed in as z) and the PLL update on a pilot position, restated from k_stepmf.hip:89-108 and :119-133.  They are
// written twice on purpose: with the two moved into a header that both files include, the device code of stepmf_kernel changes (tools/isa_same.py against the build
// before: different from instruction 542 of 2106), and that kernel stays as it is.  Whoever edits one edits the other; the GPU tests compare the two kernels' outputs.
__device__ __forceinline__ void smf_filter(const float2 *w, const float2 z, const float *taps, float &mr, float &mi)
{
    float ar[4], ai[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float2 a = w[j], c = j == 0 ? z : w[80 - j];
        ar[j] = taps[j] * (a.x + c.x);
        ai[j] = taps[j] * (a.y + c.y);
    }
#pragma unroll
    for (int q = 4; q < 40; q += 4) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float2 a = w[q + j], c = w[80 - q - j];
            ar[j] = ar[j] + taps[q + j] * (a.x + c.x);
            ai[j] = ai[j] + taps[q + j] * (a.y + c.y);
        }
    }
    const float2 mid = w[40];
    mr = ((ar[0] + ar[1]) + (ar[2] + ar[3])) + taps[40] * mid.x;
    mi = ((ai[0] + ai[1]) + (ai[2] + ai[3])) + taps[40] * mid.y;
}

// the symbol (yr, yi) at pilot position curr_idx; returns the new nu in millionths
__device__ __forceinline__ int smf_pll(SfcState &cf, const float2 *P, int n_p, int pl_frame, int curr_idx, float yr, float yi, float pg, float ig, float sps)
{
    const int pp = (curr_idx - 2) % pl_frame;
    const float2 p2 = P[pp], pc = P[curr_idx < n_p ? curr_idx : 0];
    const float a_r = yr * p2.x - yi * p2.y, a_i = yr * p2.y + yi * p2.x;
    const float b_r = cf.pprev[0] * pc.x - cf.pprev[1] * pc.y, b_i = cf.pprev[0] * pc.y + cf.pprev[1] * pc.x;
    const float phase_error = a_i * b_r - a_r * b_i;
    cf.lfs = cf.lfs + phase_error * ig;
    cf.ifs = cf.ifs + cf.dds;
    cf.dds = phase_error * pg + cf.lfs;
    cf.est = cf.ifs / sps;
    float fk = floorf(-cf.est * 1e6f);
    if (fk > 1e9f) fk = 1e9f;
    if (fk < -1e9f) fk = -1e9f;
    cf.pprev[0] = cf.prev[0]; cf.pprev[1] = cf.prev[1];
    cf.prev[0] = yr; cf.prev[1] = yi;
    return (int)fk;
}

__global__ void __launch_bounds__(64)
stepmf_wave_kernel(const float2 *__restrict__ X, float2 *__restrict__ Y, int2 *__restrict__ B, float *__restrict__ MU, float *__restrict__ FRQ, float *__restrict__ PHS,
                   const int32_t *__restrict__ DEL, const int32_t *__restrict__ ccnt, const StmState *__restrict__ st_in, StmState *__restrict__ st_out,
                   const SfcState *__restrict__ cf_in, SfcState *__restrict__ cf_out, const float2 *__restrict__ hist_in, float2 *__restrict__ hist_out,
                   const float *__restrict__ taps, const float2 *__restrict__ P, int n_p, int S, int Fs, int N, int pl_frame, float kp, float ki, float pg, float ig, float sps)
{
    __shared__ float2 zb[SMW_H + SMW_C];
    const int lane = threadIdx.x;
    const int s = blockIdx.x;
    if (s >= S) return;
    const long long L = (long long)Fs * N;                     // complex samples per stream in this call
    const float2 *x = X + (size_t)s * (size_t)L;
    float2 *y = Y + (size_t)s * (size_t)L;
    int2 *b = B + (size_t)s * (size_t)L;

    StmState st = st_in[s];
    SfcState cf = cf_in[s];
    const int carry_cplx = ccnt[s] / 2;                         // Synchronizer_timing::get_delay() = outbuf_cur_sz / 2
    GardnerRegs g;
    g.load(st);
    int n = cf.n, nu_k = cf.nu_k, curr_idx = cf.curr_idx;
    int to_frame_end = N;                                       // samples left in the current frame
    int frame = 0;
    const int N_out = 2 * N;

    // the filter's memory: 80 rotated samples, oldest first
    for (int j = lane; j < SMW_H; j += 64) zb[j] = hist_in[(size_t)s * SMW_H + j];
    const float2 zero = make_float2(0.f, 0.f);
    float2 xr = lane < L ? x[lane] : zero;                      // the chunk's raw samples

    for (long long t = 0; t < L;) {
        const int c = L - t < SMW_C ? (int)(L - t) : SMW_C;
        // AHEAD.  The phase of lane i is nco_turn_index(nu_k, (n + i) mod 1e6) = (p0 + i kmod) mod 1e6: kmod 1e6 is a whole number of turns, so the counter's wrap drops out
        int kmod = nu_k % NCO_TURN_UNITS;
        if (kmod < 0) kmod += NCO_TURN_UNITS;
        const int p = (int)(((unsigned)nco_turn_index(nu_k, n) + (unsigned)lane * (unsigned)kmod) % (unsigned)NCO_TURN_UNITS);      // < 65e6: no overflow
        float cs, sn;
        nco_turn_cs(p, &cs, &sn);
        const float2 z = make_float2(xr.x * cs - xr.y * sn, xr.x * sn + xr.y * cs);
        zb[SMW_H + lane] = z;
        __syncthreads();
        float mr, mi;
        smf_filter(zb + lane, z, taps, mr, mi);
        const float2 xn = t + SMW_C + lane < L ? x[t + SMW_C + lane] : zero;       // the next chunk's, if this one is not cut

        // LOOP
        unsigned long long m = 0ull;
        float oyr = 0.f, oyi = 0.f;
        int fin = c;
        for (int i = 0; i < c; i++) {
            if (to_frame_end == N) {                            // a frame starts: Synchronizer_step_mf_cc.cpp:189-191
                curr_idx = (N_out - DEL[(size_t)s * Fs + frame] + cf.last_delay) % (N_out / 2);
                cf.last_delay = carry_cplx;
            }
            // 3. the timing step
            float yr, yi;
            g.farrow(smw_lane(mr, i), smw_lane(mi, i), yr, yi);
            const int strobe = __builtin_amdgcn_readfirstlane(gardner_step(g, yr, yi, kp, ki));
            g.is = __builtin_amdgcn_readfirstlane(g.is);
            if (lane == i) { oyr = yr; oyi = yi; }
            m |= (unsigned long long)strobe << i;
            // 4. the PLL
            bool cut = false;
            if (strobe) {
                const int rem_pos = curr_idx % 1476;
                if (curr_idx >= 1530 && rem_pos >= 54 && rem_pos < 90) {
                    const int k1 = smf_pll(cf, P, n_p, pl_frame, curr_idx, yr, yi, pg, ig, sps);
                    if (k1 != nu_k) { nu_k = k1; cut = true; }
                } else if (curr_idx >= 1530 && rem_pos == 90) {
                    cf.pprev[0] = cf.pprev[1] = cf.prev[0] = cf.prev[1] = 0.f;
                }
                curr_idx = (curr_idx + 1) % pl_frame;
            }
            if (--to_frame_end == 0) {
                const size_t o = (size_t)s * Fs + frame;
                if (lane == 0) { MU[o] = g.mu; FRQ[o] = cf.est; PHS[o] = 0.f; }
                frame++;
                to_frame_end = N;
            }
            if (cut) { fin = i + 1; break; }                    // CUT: what lies behind sample i was rotated with the old nu
        }
        if (lane < fin) {
            const int f = (int)((m >> lane) & 1ull);
            y[t + lane] = make_float2(oyr, oyi);
            b[t + lane] = make_int2(f, f);
        }
        // the window moves on by the final samples: fin + 79 <= 143
        const float2 h0 = zb[fin + lane], h1 = zb[fin + (lane < SMW_H - 64 ? 64 + lane : 0)];
        __syncthreads();
        zb[lane] = h0;
        if (lane < SMW_H - 64) zb[64 + lane] = h1;
        n += fin;
        if (n >= NCO_TURN_UNITS) n -= NCO_TURN_UNITS;
        t += fin;
        xr = fin == SMW_C ? xn : t + lane < L ? x[t + lane] : zero;
    }
    __syncthreads();
    for (int j = lane; j < SMW_H; j += 64) hist_out[(size_t)s * SMW_H + j] = zb[j];
    if (lane == 0) {
        g.store(st);
        st_out[s] = st;
        cf.n = n; cf.nu_k = nu_k; cf.curr_idx = curr_idx;
        cf_out[s] = cf;
    }
}

hipError_t stepmf_wave_launch(const float *X, float *Y, int32_t *B, float *MU, float *FRQ, float *PHS, const int32_t *DEL, const int32_t *ccnt, const StmState *st_in,
                              StmState *st_out, const SfcState *cf_in, SfcState *cf_out, const float *hist_in, float *hist_out, const float *taps, const float *P, int n_p, int S,
                              int Fs, int N, int pl_frame, float kp, float ki, float pg, float ig, float sps, hipStream_t s)
{
    hipLaunchKernelGGL(stepmf_wave_kernel, dim3((unsigned)S), dim3(64), 0, s, reinterpret_cast<const float2 *>(X), reinterpret_cast<float2 *>(Y),
                       reinterpret_cast<int2 *>(B), MU, FRQ, PHS, DEL, ccnt, st_in, st_out, cf_in, cf_out, reinterpret_cast<const float2 *>(hist_in),
                       reinterpret_cast<float2 *>(hist_out), taps, reinterpret_cast<const float2 *>(P), n_p, S, Fs, N, pl_frame, kp, ki, pg, ig, sps);
    return hipGetLastError();
}

}  // namespace dvbs2
