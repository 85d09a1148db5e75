/*
 * stepmf_twin.c -- CPU twin of the fused coarse-frequency / matched-filter / timing loop (the reference's Synchronizer_step_mf_cc).  TEST INFRASTRUCTURE ONLY:
 * tests/stepmf_ref.py compiles it with the system compiler (-O2 -ffp-contract=off, so that no product is fused into a sum) and loads it with ctypes; the GPU tests hold
 * k_stepmf.hip to it bit for bit.  Written from the algorithm, one stream at a time, in the reference's order.  Citations are relative to the reference's src/common/.
 *
 * Two things are this project's own choice, not the reference's, and both are part of the contract with the kernel:
 *   - the rotation: cos / sin of the exact turn fraction (k n mod 1e6) / 1e6 by dvbs2_amd/csrc/nco_turn.h, where the reference takes std::cos / std::sin of the fp32
 *     product omega n (Multiplier_sine_ccc_naive.cpp:71-72);
 *   - the matched filter's order of additions.  With w[0] the oldest and w[80] the newest of the 81 rotated samples and t[] the taps (t[i] == t[80 - i], checked):
 *         a_j = sum over i = j, j + 4, j + 8, .. <= 39, in increasing i, of t[i] * (w[i] + w[80 - i])        (j = 0 .. 3; the first term starts the sum)
 *         y   = ((a_0 + a_1) + (a_2 + a_3)) + t[40] * w[40]
 *     real and imaginary part alike: 41 products.  The reference sums the 81 products oldest first (Filter_FIR_ccr_naive.hpp:36-49).
 */
#include <math.h>
#include <string.h>
#include <stdlib.h>
#include "../dvbs2_amd/csrc/nco_turn.h"
#include "gardner_twin.h"

#define MF_T 81

/* the coarse synchronizer's state (Synchronizer_freq_coarse_DVBS2_aib + its Multiplier_sine_ccc_naive) and Synchronizer_step_mf_cc::last_delay */
typedef struct {
    float prev[2], pprev[2];      /* prev_spl, prev_prev_spl */
    float lfs, ifs, dds;          /* loop_filter_state, integ_filter_state, DDS_prev_in */
    float est;                    /* estimated_freq */
    int nu_k;                     /* the multiplier's nu in millionths: nu = nu_k / 1e6 (set_nu floors to six decimals) */
    int n;                        /* the multiplier's sample counter, 0 .. 999999 */
    int curr_idx;
    int last_delay;
} twin_sfc;

/* Synchronizer_freq_coarse_DVBS2_aib::set_PLL_coeffs, Module/Synchronizer/Synchronizer_freq/Synchronizer_freq_coarse/Synchronizer_freq_coarse_DVBS2_aib.cpp:94-113, R = float:
 * the 0.25 is a double constant there, so (damping + 0.25 / damping) is a double sum and the quotient is rounded to float once */
void twin_pll_gains(int pll_sps, float damping, float nbw, float *pg, float *ig)
{
    float det_gain = 2.0f;
    float bw = nbw * (float)pll_sps;
    float K0 = (float)pll_sps;
    float theta = (float)((double)bw / (((double)damping + 0.25 / (double)damping) * (double)(float)pll_sps));
    float d = 1.0f + 2.0f * damping * theta + theta * theta;
    *pg = (4.0f * damping * theta / d) / (det_gain * K0);
    *ig = (4.0f / (float)pll_sps * theta * theta / d) / (det_gain * K0);
}

/* scrambled_pilots, .cpp:28-31: entry i < 90 is 0, else exp(j pi/2 (R[i - 90] + 0.5)); (R)M_PI_2 is a float, the sum a double, std::cos / std::sin of a double, rounded to
 * float.  seq: the PL scrambling sequence R (n_seq values 0 .. 3); P: n_p complex entries; entries past 90 + n_seq are 0 (the reference's table ends there) */
void twin_pilots(const unsigned char *seq, int n_seq, float *P, int n_p)
{
    const float pi_2 = 1.57079632679489661923132169163975144f;
    for (int i = 0; i < n_p; i++) {
        if (i < 90 || i - 90 >= n_seq) { P[2 * i] = 0.f; P[2 * i + 1] = 0.f; continue; }
        const double a = (double)pi_2 * ((double)(float)seq[i - 90] + 0.5);
        P[2 * i] = (float)cos(a);
        P[2 * i + 1] = (float)sin(a);
    }
}

/* Synchronizer_freq_coarse_DVBS2_aib::update_phase, .cpp:57-92, with Multiplier_sine_ccc_naive::set_nu (Module/Multiplier/Sine/Multiplier_sine_ccc_naive.cpp:43-51) */
static void update_phase(twin_sfc *c, float sr, float si, const float *P, int n_p, int length_max, float pg, float ig, float sps)
{
    const int rem_pos = c->curr_idx % 1476;
    if (rem_pos >= 54 && rem_pos < 90 && c->curr_idx >= 1530) {
        const int pp = (c->curr_idx - 2) % length_max;
        const int ci = c->curr_idx < n_p ? c->curr_idx : 0;                  /* (entry 0 is zero, like everything the table does not hold) */
        const float p2r = P[2 * pp], p2i = P[2 * pp + 1], pcr = P[2 * ci], pci = P[2 * ci + 1];
        const float ar = sr * p2r - si * p2i, ai = sr * p2i + si * p2r;      /* spl * scrambled_pilots[prev_prev_idx] */
        const float br = c->pprev[0] * pcr - c->pprev[1] * pci, bi = c->pprev[0] * pci + c->pprev[1] * pcr;      /* prev_prev_spl * scrambled_pilots[curr_idx] */
        const float phase_error = ai * br - ar * bi;                         /* imag(a * conj(b)) */
        c->lfs += phase_error * ig;                                          /* :72 */
        c->ifs += c->dds;                                                    /* :74 */
        c->dds = phase_error * pg + c->lfs;                                  /* :76 */
        c->est = c->ifs / sps;                                               /* :78, digital_synthesizer_gain = 1 */
        float fk = floorf(-c->est * 1e6f);                                   /* set_nu(-estimated_freq): new_nu = floor(nu 1e6) / 1e6 */
        if (fk > 1e9f) fk = 1e9f;
        if (fk < -1e9f) fk = -1e9f;                                          /* (the int below must hold it; |nu| > 1000 cycles per sample is not a frequency) */
        c->nu_k = (int)fk;
        c->pprev[0] = c->prev[0]; c->pprev[1] = c->prev[1];
        c->prev[0] = sr; c->prev[1] = si;
    } else if (rem_pos == 90 && c->curr_idx >= 1530) {
        c->pprev[0] = c->pprev[1] = c->prev[0] = c->prev[1] = 0.f;
    }
    c->curr_idx = (c->curr_idx + 1) % length_max;
}

/* Synchronizer_step_mf_cc::synchronize / _synchronize (Module/Synchronizer/Synchronizer_step_mf_cc.cpp:163-208) over n_frames frames of N complex samples of ONE stream.
 *   ring     : the matched filter's memory, the last 80 rotated samples, oldest first (2 * 80 floats)
 *   taps     : the 81 taps;  P, n_p: twin_pilots' table
 *   DEL      : the frame synchronizer's delay per frame;  carry_cplx: Synchronizer_timing::get_delay() when the call starts (reals held by extract's buffer / 2)
 *   pl_frame : length_max = N_in / (2 sps) symbols (.cpp:20);  N = pl_frame * 2
 * The timing step is Synchronizer_Gardner_fast_osf2::step (Module/Synchronizer/Synchronizer_timing/Synchronizer_Gardner_fast_osf2.hxx:8-87) as it is written there -- not
 * the _synchronize body that tests/timing_twin.c restates: TED_update's case 1 zeroes TED_buffer[0] where _synchronize shifts, cases 2 and 3 both shift where _synchronize's
 * case 3 zeroes, the loop filter is evaluated with TED_error = 0 off the strobes, and the NCO is (NCO + 1) - W where _synchronize has NCO + (1 - W). */
void twin_stepmf(twin_stm *st, twin_sfc *c, float *ring, const float *taps, const float *P, int n_p, const int *DEL, int carry_cplx,
                 const float *X, float *Y, int *B, float *MU, float *FRQ, float *PHS, int n_frames, int N, int pl_frame, float kp, float ki, float pg, float ig, float sps)
{
    float *w = (float *)malloc(sizeof(float) * 2 * (size_t)(MF_T - 1 + N));
    float b[3];
    farrow_taps(st->mu, b);
    int kmod = c->nu_k % NCO_TURN_UNITS;
    if (kmod < 0) kmod += NCO_TURN_UNITS;
    int p = nco_turn_index(c->nu_k, c->n);
    const int N_out = 2 * N;                                               /* sync_timing->get_N_in(): reals */
    for (int f = 0; f < n_frames; f++) {
        /* _synchronize, :189-191 */
        c->curr_idx = (N_out - DEL[f] + c->last_delay) % (N_out / 2);
        c->last_delay = carry_cplx;
        memcpy(w, ring, sizeof(float) * 2 * (MF_T - 1));
        for (int i = 0; i < N; i++) {
            const long long k = (long long)f * N + i;
            const float xr = X[2 * k], xi = X[2 * k + 1];
            /* sync_coarse_f->step = Multiplier_sine_ccc_naive::step */
            float cs, sn;
            nco_turn_cs(p, &cs, &sn);
            float *wi = w + 2 * i;
            wi[2 * (MF_T - 1)] = xr * cs - xi * sn;
            wi[2 * (MF_T - 1) + 1] = xr * sn + xi * cs;
            c->n = c->n >= 999999 ? 0 : c->n + 1;
            p += kmod;
            if (p >= NCO_TURN_UNITS) p -= NCO_TURN_UNITS;
            /* matched_filter->step, in the order of this file's header */
            float ar[4], ai[4];
            for (int j = 0; j < 4; j++) {
                ar[j] = taps[j] * (wi[2 * j] + wi[2 * (80 - j)]);
                ai[j] = taps[j] * (wi[2 * j + 1] + wi[2 * (80 - j) + 1]);
            }
            for (int q = 4; q < 40; q += 4)
                for (int j = 0; j < 4; j++) {
                    ar[j] = ar[j] + taps[q + j] * (wi[2 * (q + j)] + wi[2 * (80 - q - j)]);
                    ai[j] = ai[j] + taps[q + j] * (wi[2 * (q + j) + 1] + wi[2 * (80 - q - j) + 1]);
                }
            const float mr = ((ar[0] + ar[1]) + (ar[2] + ar[3])) + taps[40] * wi[80];
            const float mi = ((ai[0] + ai[1]) + (ai[2] + ai[3])) + taps[40] * wi[81];
            /* sync_timing->step, Synchronizer_Gardner_fast_osf2.hxx:8-21: farrow_flt.step */
            float yr, yi;
            farrow(st, b, mr, mi, &yr, &yi);
            Y[2 * k] = yr; Y[2 * k + 1] = yi;
            const int strobe = st->is_strobe;
            B[2 * k] = strobe; B[2 * k + 1] = strobe;
            if (strobe == 1) { st->last[0] = yr; st->last[1] = yi; }
            /* TED_update, .hxx:55-87 */
            const int hist = st->is_strobe + st->prev_is_strobe * 2;
            float e = 0.0f;
            if (hist == 1) e = st->ted[2] * (st->ted[0] - yr) + st->ted[3] * (st->ted[1] - yi);
            if (hist == 1) {
                st->ted[0] = 0.f; st->ted[1] = 0.f; st->ted[2] = yr; st->ted[3] = yi;
            } else if (hist != 0) {
                st->ted[0] = st->ted[2]; st->ted[1] = st->ted[3]; st->ted[2] = yr; st->ted[3] = yi;
            }
            /* loop_filter, .hxx:23-35 */
            const float vp = e * kp;
            const float vi = st->lf_prev_in + e * ki;
            st->lf_prev_in = vi;
            st->lf_output = vp + vi;
            /* interpolation_control, .hxx:37-53 */
            const float W = st->lf_output + 0.5f;
            st->prev_is_strobe = st->is_strobe;
            st->is_strobe = st->nco < W ? 1 : 0;
            if (st->is_strobe == 1) {
                st->mu = st->nco / W;
                farrow_taps(st->mu, b);
                st->nco += 1.0f;
            }
            st->nco = st->nco - W;
            /* Synchronizer_step_mf_cc.cpp:205-206 */
            if (strobe == 1) {
                const int k0 = c->nu_k;
                update_phase(c, st->last[0], st->last[1], P, n_p, pl_frame, pg, ig, sps);
                if (c->nu_k != k0) {
                    kmod = c->nu_k % NCO_TURN_UNITS;
                    if (kmod < 0) kmod += NCO_TURN_UNITS;
                    p = nco_turn_index(c->nu_k, c->n);
                }
            }
        }
        memcpy(ring, w + 2 * N, sizeof(float) * 2 * (MF_T - 1));
        MU[f] = st->mu;                 /* :177-179 */
        FRQ[f] = c->est;
        PHS[f] = 0.f;                   /* estimated_phase: set to 0 by reset() and never written (Synchronizer_freq_coarse.hxx:60-67) */
    }
    free(w);
}

/* the worst |error| of nco_turn_cs against double-precision cos / sin over all 1e6 arguments */
double twin_nco_turn_worst(void)
{
    double worst = 0.0;
    for (int p = 0; p < NCO_TURN_UNITS; p++) {
        float c, s;
        nco_turn_cs(p, &c, &s);
        const double a = 6.283185307179586476925286766559 * (double)p / 1e6;
        const double ec = fabs((double)c - cos(a)), es = fabs((double)s - sin(a));
        if (ec > worst) worst = ec;
        if (es > worst) worst = es;
    }
    return worst;
}

void twin_nco_turn(int p, float *c, float *s) { nco_turn_cs(p, c, s); }
int twin_nco_index(int k, int n) { return nco_turn_index(k, n); }
