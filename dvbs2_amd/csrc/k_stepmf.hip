// The coarse-frequency loop: the reference's Synchronizer_step_mf_cc (src/common/Module/Synchronizer/Synchronizer_step_mf_cc.cpp:163-208), the task of its waiting and
// learning phases 1-2 (src/mains/RX/main_sched.cpp:407-560).  Per complex input sample, in this order:
//   1. Synchronizer_freq_coarse_DVBS2_aib::step = Multiplier_sine_ccc_naive::step (Multiplier_sine_ccc_naive.cpp:67-75): z = x (cos + j sin)(2 pi nu n), n counts 0 .. 999999
//   2. Filter_FIR_ccr_naive::step (Filter_FIR_ccr_naive.hpp:36-49): the 81-tap matched filter over the last 81 rotated samples
//   3. Synchronizer_Gardner_fast_osf2::step (Synchronizer_Gardner_fast_osf2.hxx:8-87): Farrow interpolator, Gardner detector, PI loop filter, NCO
//   4. on a strobe, Synchronizer_freq_coarse_DVBS2_aib::update_phase (.cpp:57-92) with the symbol just interpolated: on pilot positions the detector
//      Im(spl P[idx-2] conj(prev_prev_spl P[idx])), the PI filter, the integrator, estimated_freq = integ / sps, set_nu(-estimated_freq) floored to six decimals
// and once per frame curr_idx = (N_out - DEL + last_delay) mod (N_out / 2) from the frame synchronizer's fed-back delay (:189-191).
// Everything depends on the sample before: the new nu rotates the next sample, which enters the filter, whose output moves the strobe.  So, as in k_timing.hip, ONE LANE PER
// STREAM, stream-major frames, and tiles of the 64 streams' samples staged through LDS so that global loads and stores stay coalesced.
//
// Arithmetic contract (tests/stepmf_twin.c, bit for bit): the rotation takes cos / sin of the exact turn fraction (k n mod 1e6) / 1e6 from nco_turn.h -- nu = k 1e-6 and n
// are whole numbers, so nothing is rounded before the polynomial; the matched filter uses the taps' symmetry, 41 products summed in the order the twin's header states; the
// timing step is Synchronizer_Gardner_fast_osf2::step as written: gardner_step of gardner_loop.h, which lists how it differs from the _synchronize body of k_timing.hip.
//
// LDS: a lane's row holds its filter window and its tile in one run of float2: [80 samples of history | T new samples].  Sample i of the tile is rotated in place at
// row[80 + i], the filter reads row[i .. i + 80], and the interpolated output goes to row[i], which no later sample reads.  After the tile the last 80 samples move to the
// front.  The row stride is SMF_ROW = 125 float2 = 250 dwords: twice an odd number, so the 32 lanes that one ds_read_b64 serves together (bank = dword mod 64) and the 16
// that a ds_write_b64 serves together (mod 32) all sit on different banks on their lane-private walks.  64 x 125 x 8 B = 62.5 KB + 512 B of strobe masks per workgroup of
// one wave: two workgroups per CU (160 KB).  Nothing of the window lives in scratch.
#include "gardner_loop.h"
#include "nco_turn.h"

namespace dvbs2 {

constexpr int SMF_T = 44;                          // samples per stream and tile
constexpr int SMF_H = 80;                          // the matched filter's memory: taps - 1
constexpr int SMF_ROW = SMF_H + SMF_T + 1;         // float2 per LDS row: 125, odd

__global__ void __launch_bounds__(64)
stepmf_kernel(const float2 *__restrict__ X, float2 *__restrict__ Y, int2 *__restrict__ B, float *__restrict__ MU, float *__restrict__ FRQ, float *__restrict__ PHS,
              const int32_t *__restrict__ DEL, const int32_t *__restrict__ ccnt, const StmState *__restrict__ st_in, StmState *__restrict__ st_out,
              const SfcState *__restrict__ cf_in, SfcState *__restrict__ cf_out, const float2 *__restrict__ hist_in, float2 *__restrict__ hist_out,
              const float *__restrict__ taps, const float2 *__restrict__ P, int n_p, int S, int Fs, int N, int pl_frame, float kp, float ki, float pg, float ig, float sps)
{
    __shared__ float2 tile[64 * SMF_ROW];
    __shared__ unsigned long long msk[64];
    const int lane = threadIdx.x;
    const int s0 = blockIdx.x * 64;
    const int rows = S - s0 < 64 ? S - s0 : 64;
    const int s = s0 + lane;
    const bool act = lane < rows;
    const long long L = (long long)Fs * N;                     // complex samples per stream in this call

    StmState st = {};
    SfcState cf = {};
    int carry_cplx = 0;
    if (act) { st = st_in[s]; cf = cf_in[s]; carry_cplx = ccnt[s] / 2; }          // Synchronizer_timing::get_delay() = outbuf_cur_sz / 2
    GardnerRegs g;
    g.load(st);
    int n = cf.n, nu_k = cf.nu_k, curr_idx = cf.curr_idx;
    int kmod = nu_k % NCO_TURN_UNITS;
    if (kmod < 0) kmod += NCO_TURN_UNITS;
    int p = nco_turn_index(nu_k, n);
    int to_frame_end = N;                                       // samples left in the current frame
    int frame = 0;
    const int N_out = 2 * N;
    float2 *row = tile + lane * SMF_ROW;

    // the filter's memory: 80 samples per stream, oldest first
    for (int r = 0; r < rows; r++)
        for (int j = lane; j < SMF_H; j += 64) tile[r * SMF_ROW + j] = hist_in[(size_t)(s0 + r) * SMF_H + j];
    __syncthreads();

    for (long long t0 = 0; t0 < L; t0 += SMF_T) {
        const int cnt = L - t0 < SMF_T ? (int)(L - t0) : SMF_T;
        if (lane < cnt) {
#pragma unroll 8
            for (int r = 0; r < rows; r++) tile[r * SMF_ROW + SMF_H + lane] = X[(size_t)(s0 + r) * (size_t)L + (size_t)t0 + lane];
        }
        __syncthreads();
        if (act) {
            unsigned long long m = 0ull;
            for (int i = 0; i < cnt; i++) {
                if (to_frame_end == N) {                        // a frame starts: Synchronizer_step_mf_cc.cpp:189-191
                    curr_idx = (N_out - DEL[(size_t)s * Fs + frame] + cf.last_delay) % (N_out / 2);
                    cf.last_delay = carry_cplx;
                }
                float2 *w = row + i;
                // 1. the rotation
                float cs, sn;
                nco_turn_cs(p, &cs, &sn);
                const float2 x = w[SMF_H];
                const float2 z = make_float2(x.x * cs - x.y * sn, x.x * sn + x.y * cs);
                w[SMF_H] = z;
                n = n >= 999999 ? 0 : n + 1;
                p += kmod;
                if (p >= NCO_TURN_UNITS) p -= NCO_TURN_UNITS;
                // 2. the matched filter: four interleaved partial sums over the 40 symmetric pairs, then the centre tap
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
                const float mr = ((ar[0] + ar[1]) + (ar[2] + ar[3])) + taps[40] * mid.x;
                const float mi = ((ai[0] + ai[1]) + (ai[2] + ai[3])) + taps[40] * mid.y;
                // 3. the timing step
                float yr, yi;
                g.farrow(mr, mi, yr, yi);
                const int strobe = gardner_step(g, yr, yi, kp, ki);
                w[0] = make_float2(yr, yi);
                m |= (unsigned long long)strobe << i;
                // 4. the PLL
                if (strobe) {
                    const int rem_pos = curr_idx % 1476;
                    if (curr_idx >= 1530 && rem_pos >= 54 && rem_pos < 90) {
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
                        const int k1 = (int)fk;
                        cf.pprev[0] = cf.prev[0]; cf.pprev[1] = cf.prev[1];
                        cf.prev[0] = yr; cf.prev[1] = yi;
                        if (k1 != nu_k) {
                            nu_k = k1;
                            kmod = nu_k % NCO_TURN_UNITS;
                            if (kmod < 0) kmod += NCO_TURN_UNITS;
                            p = nco_turn_index(nu_k, n);
                        }
                    } else if (curr_idx >= 1530 && rem_pos == 90) {
                        cf.pprev[0] = cf.pprev[1] = cf.prev[0] = cf.prev[1] = 0.f;
                    }
                    curr_idx = (curr_idx + 1) % pl_frame;
                }
                if (--to_frame_end == 0) {
                    const size_t o = (size_t)s * Fs + frame;
                    MU[o] = g.mu; FRQ[o] = cf.est; PHS[o] = 0.f;
                    frame++;
                    to_frame_end = N;
                }
            }
            msk[lane] = m;
        }
        __syncthreads();
        if (lane < cnt) {
#pragma unroll 8
            for (int r = 0; r < rows; r++) {
                const size_t o = (size_t)(s0 + r) * (size_t)L + (size_t)t0 + lane;
                Y[o] = tile[r * SMF_ROW + lane];
                const int f = (int)((msk[r] >> lane) & 1ull);
                B[o] = make_int2(f, f);
            }
        }
        __syncthreads();
        if (act) {                                              // the window moves on: the last 80 samples to the front (ascending: a slot is read before it is overwritten)
            for (int j = 0; j < SMF_H; j++) row[j] = row[j + cnt];
        }
        __syncthreads();
    }
    for (int r = 0; r < rows; r++)
        for (int j = lane; j < SMF_H; j += 64) hist_out[(size_t)(s0 + r) * SMF_H + j] = tile[r * SMF_ROW + j];
    if (act) {
        g.store(st);
        st_out[s] = st;
        cf.n = n; cf.nu_k = nu_k; cf.curr_idx = curr_idx;
        cf_out[s] = cf;
    }
}

hipError_t stepmf_launch(const float *X, float *Y, int32_t *B, float *MU, float *FRQ, float *PHS, const int32_t *DEL, const int32_t *ccnt, const StmState *st_in, StmState *st_out,
                         const SfcState *cf_in, SfcState *cf_out, const float *hist_in, float *hist_out, const float *taps, const float *P, int n_p, int S, int Fs, int N, int pl_frame,
                         float kp, float ki, float pg, float ig, float sps, hipStream_t s)
{
    hipLaunchKernelGGL(stepmf_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, s, reinterpret_cast<const float2 *>(X), reinterpret_cast<float2 *>(Y),
                       reinterpret_cast<int2 *>(B), MU, FRQ, PHS, DEL, ccnt, st_in, st_out, cf_in, cf_out, reinterpret_cast<const float2 *>(hist_in),
                       reinterpret_cast<float2 *>(hist_out), taps, reinterpret_cast<const float2 *>(P), n_p, S, Fs, N, pl_frame, kp, ki, pg, ig, sps);
    return hipGetLastError();
}

}  // namespace dvbs2
