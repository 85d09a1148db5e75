/*
 * timing_twin.c -- CPU twin of the timing synchronizer and the channel's delay tasks.  TEST INFRASTRUCTURE ONLY: tests/test_timing_twin.py compiles it with the system compiler
 * (-O2 -ffp-contract=off, so that no product is fused into a sum) and loads it with ctypes; the GPU tests hold libdvbs2hip's kernels to it bit for bit.
 * Written from the algorithm, one stream at a time, in the reference's order.  Citations are relative to the reference's src/common/.
 */
#include <math.h>
#include <string.h>
#include "gardner_twin.h"

/* Synchronizer_Gardner_fast_osf2::set_loop_filter_coeffs, Module/Synchronizer/Synchronizer_timing/Synchronizer_Gardner_fast_osf2.cpp:188-198 */
void twin_gains(float damping, float nbw, float dg, float *kp, float *ki) { loop_gains(damping, nbw, dg, kp, ki); }

/* Synchronizer_timing::synchronize (Synchronizer_timing.hxx:189-201) over n_frames frames of N complex samples of ONE stream,
 * each frame Synchronizer_Gardner_fast_osf2::_synchronize (.cpp:35-166) with the Farrow step of Filter_Farrow_ccr_naive.hxx */
void twin_synchronize(twin_stm *st, const float *X, float *Y, int *B, float *MU, int n_frames, int N, float kp, float ki)
{
    float b[3];
    farrow_taps(st->mu, b);
    for (int f = 0; f < n_frames; f++) {
        for (int i = 0; i < N; i++) {
            const long long k = (long long)f * N + i;
            const float xr = X[2 * k], xi = X[2 * k + 1];
            const int hist = st->is_strobe + st->prev_is_strobe * 2;          /* strobe_history, .cpp:44,68 */
            /* farrow_flt.step (in every branch; the set_mu(mu) of branch 3, .cpp:116, sets the taps they already hold) */
            float yr, yi;
            farrow(st, b, xr, xi, &yr, &yi);
            Y[2 * k] = yr; Y[2 * k + 1] = yi;
            const int strobe = hist == 1 || hist == 3;
            B[2 * k] = strobe; B[2 * k + 1] = strobe;
            if (strobe) { st->last[0] = yr; st->last[1] = yi; }
            if (hist == 1) {                                                   /* .cpp:47-80 */
                const float e = st->ted[2] * (st->ted[0] - yr) + st->ted[3] * (st->ted[1] - yi);
                st->lf_prev_in += e * ki;
                st->lf_output = st->lf_prev_in + e * kp;
                st->ted[0] = st->ted[2]; st->ted[1] = st->ted[3]; st->ted[2] = yr; st->ted[3] = yi;
            } else if (hist == 2) {                                            /* .cpp:81-110 */
                st->ted[0] = st->ted[2]; st->ted[1] = st->ted[3]; st->ted[2] = yr; st->ted[3] = yi;
                st->lf_output = st->lf_prev_in;
            } else if (hist == 3) {                                            /* .cpp:111-142 */
                st->ted[0] = 0.f; st->ted[1] = 0.f; st->ted[2] = yr; st->ted[3] = yi;
                st->lf_output = st->lf_prev_in;
            } else {                                                           /* .cpp:143-164 */
                st->lf_output = st->lf_prev_in;
            }
            const float W = st->lf_output + 0.5f;
            st->prev_is_strobe = st->is_strobe;
            st->is_strobe = st->nco < W;
            if (st->is_strobe) {
                st->mu = st->nco / W;
                farrow_taps(st->mu, b);
                st->nco += 1.0f - W;
            } else {
                st->nco -= W;
            }
        }
        MU[f] = st->mu;
    }
}

/* Synchronizer_timing::extract / _extract (Synchronizer_timing.hxx:243-304) for ONE stream of n_frames frames: N complex samples (2 N reals) in, N reals out per frame.
 * carry: `cap` reals, *head of them held (the reference grows its buffer; here the reals past `cap` are dropped, as libdvbs2hip does); uf[n_frames]: the underflow counts.
 * Returns 1 when the stream is ready (2: ready, but reals past `cap` were dropped), 0 on an underflow (where the reference throws processing_aborted: its UFW is then written by the next call, which this one's UFW
 * anticipates -- UFW = the counts since the last ready call, this one's included; a ready call clears them). */
int twin_extract(float *carry, long long *head, long long cap, int *uf, const float *Y1, const int *B1, float *Y2, int *UFW, int n_frames, int N)
{
    const long long M = (long long)N * n_frames;
    const long long tmp = *head < M ? *head : M;
    memcpy(Y2, carry, sizeof(float) * (size_t)tmp);
    memmove(carry, carry + tmp, sizeof(float) * (size_t)(*head - tmp));
    long long h = *head - tmp, n = tmp;
    for (long long i = 0; i < 2LL * N * n_frames; i++) {
        if (B1[i]) {
            if (n < M) Y2[n++] = Y1[i];
            else { if (h < cap) carry[h] = Y1[i]; h++; }
        }
    }
    int ready = 1;
    if (n < M) {
        memcpy(carry, Y2, sizeof(float) * (size_t)n);
        h += n;
        uf[n / N]++;
        ready = 0;
    }
    if (ready && h > cap) ready = 2;                     /* ready, but the carry buffer lost h - cap reals */
    *head = h < cap ? h : cap;
    for (int f = 0; f < n_frames; f++) {
        UFW[f] = uf[f];
        if (ready) uf[f] = 0;
    }
    return ready;
}

/* the channel's delay tasks for --chn-max-delay D (Factory/DVBS2/DVBS2.cpp:520-544), bound frame delay -> integer delay -> fractional delay (mains/CH/main.cpp:60-62):
 * Filter_buffered_delay ((floor(D) - 2) / N frames, Module/Filter/Filter_unit_delay/Filter_buffered_delay.cpp) and Variable_delay_cc_naive ((floor(D) - 2 + N) % N samples,
 * Module/Filter/Variable_delay/Variable_delay_cc_naive.cpp) start from zeros; together they delay by floor(D) - 2 samples.  Then the Farrow filter with mu = D - floor(D)
 * (Filter_FIR_ccr::_filter sums (b0 x0 + b1 x1) + (b2 x2 + b3 x3), Filter_FIR_ccr.cpp:103-128, as step() does).  hist: the last H = floor(D) + 1 samples (zeros at first). */
long long twin_channel_taps(float D, float b[3])
{
    farrow_taps(D - floorf(D), b);
    return (long long)floorf(D) + 1;
}

void twin_channel_delay(float *hist, long long H, const float b[3], const float *X, float *Y, long long T)
{
    /* z = the delayed stream, fed through the Farrow filter: history first, then X */
    for (long long n = 0; n < T; n++) {
        float c[8];
        for (int t = 0; t < 4; t++) {
            const long long j = n + t;
            const float *src = j < H ? hist + 2 * j : X + 2 * (j - H);
            c[2 * t] = src[0]; c[2 * t + 1] = src[1];
        }
        const float r0 = c[0] * b[0], r1 = c[2] * b[1], r2 = c[4] * b[2], r3 = c[6] * b[0];
        const float i0 = c[1] * b[0], i1 = c[3] * b[1], i2 = c[5] * b[2], i3 = c[7] * b[0];
        Y[2 * n] = (r0 + r1) + (r2 + r3);
        Y[2 * n + 1] = (i0 + i1) + (i2 + i3);
    }
    /* the new history: the last H samples of (history, X) */
    if (T >= H) {
        memcpy(hist, X + 2 * (T - H), sizeof(float) * 2 * (size_t)H);
    } else {
        memmove(hist, hist + 2 * T, sizeof(float) * 2 * (size_t)(H - T));
        memcpy(hist + 2 * (H - T), X, sizeof(float) * 2 * (size_t)T);
    }
}
