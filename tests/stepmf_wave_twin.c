/*
 * stepmf_wave_twin.c -- the coarse-frequency loop of stepmf_twin.c in the order of the one-wave-per-stream kernel (dvbs2_amd/csrc/k_stepmf_wave.hip).  TEST
 * INFRASTRUCTURE ONLY, built like the other twins (tests/twin_build.py: -O2 -ffp-contract=off).  stepmf_twin.c is included unchanged: the state, update_phase and the
 * Farrow step are its own; the per-sample timing step is restated from twin_stepmf, line for line.
 *
 * What differs is the ORDER, not one operation.  nu changes only in update_phase, on a strobe at a pilot position, so between two changes rotation and matched filter are a
 * feed-forward of the input.  Per stream, until the call's n_frames * N samples are done:
 *   chunk : the next c = min(64, samples left) samples behind the last final one
 *   ahead : for every i < c: z_i = x_i rotated by nco_turn_index(nu_k, (n + i) mod 1e6), stored behind the 80 samples of history; then for every i < c the matched filter
 *           over z[i - 80 .. i], in the order of stepmf_twin.c's header
 *   loop  : i = 0 .. c - 1: frame start, Farrow, the timing step, Y and B, on a strobe update_phase, at the frame's end MU / FRQ / PHS
 *   cut   : if update_phase at sample i changed nu_k, samples 0 .. i are final and the chunk ends there; n and the window advance by i + 1, and what lay behind is rotated
 *           and filtered again from the raw input with the new nu_k.  Otherwise all c samples are final.
 * That this gives twin_stepmf's bits (tests/test_stepmf_wave_twin.py) is the CPU statement that the scheme is exact.  The function also reports the cuts of the call, as
 * (sample index in the call, position in its chunk): what the GPU tests' inputs exercise.
 */
#include "stepmf_twin.c"

#define WV_C 64

/* twin_stepmf's arguments, then cuts: 2 * max_cuts ints, filled with (sample, position) per cut as far as there is room.  Returns the number of cuts of the call. */
int twin_stepmf_wave(twin_stm *st, twin_sfc *c, float *ring, const float *taps, const float *P, int n_p, const int *DEL, int carry_cplx,
                     const float *X, float *Y, int *B, float *MU, float *FRQ, float *PHS, int n_frames, int N, int pl_frame, float kp, float ki, float pg, float ig, float sps,
                     int *cuts, int max_cuts)
{
    float zb[2 * (MF_T - 1 + WV_C)], mr[WV_C], mi[WV_C];
    float b[3];
    farrow_taps(st->mu, b);
    memcpy(zb, ring, sizeof(float) * 2 * (MF_T - 1));
    const long long L = (long long)n_frames * N;
    const int N_out = 2 * N;
    int to_frame_end = N, frame = 0, n_cuts = 0;
    for (long long t = 0; t < L;) {
        const int cn = L - t < WV_C ? (int)(L - t) : WV_C;
        /* ahead: the rotation ... */
        for (int i = 0; i < cn; i++) {
            const float xr = X[2 * (t + i)], xi = X[2 * (t + i) + 1];
            float cs, sn;
            nco_turn_cs(nco_turn_index(c->nu_k, (c->n + i) % NCO_TURN_UNITS), &cs, &sn);
            zb[2 * (MF_T - 1 + i)] = xr * cs - xi * sn;
            zb[2 * (MF_T - 1 + i) + 1] = xr * sn + xi * cs;
        }
        /* ... and the matched filter */
        for (int i = 0; i < cn; i++) {
            const float *wi = zb + 2 * i;
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
            mr[i] = ((ar[0] + ar[1]) + (ar[2] + ar[3])) + taps[40] * wi[80];
            mi[i] = ((ai[0] + ai[1]) + (ai[2] + ai[3])) + taps[40] * wi[81];
        }
        /* loop */
        int fin = cn;
        for (int i = 0; i < cn; i++) {
            const long long k = t + i;
            if (to_frame_end == N) {                                           /* _synchronize, Synchronizer_step_mf_cc.cpp:189-191 */
                c->curr_idx = (N_out - DEL[frame] + c->last_delay) % (N_out / 2);
                c->last_delay = carry_cplx;
            }
            /* sync_timing->step, as in twin_stepmf */
            float yr, yi;
            farrow(st, b, mr[i], mi[i], &yr, &yi);
            Y[2 * k] = yr; Y[2 * k + 1] = yi;
            const int strobe = st->is_strobe;
            B[2 * k] = strobe; B[2 * k + 1] = strobe;
            if (strobe == 1) { st->last[0] = yr; st->last[1] = yi; }
            const int hist = st->is_strobe + st->prev_is_strobe * 2;
            float e = 0.0f;
            if (hist == 1) e = st->ted[2] * (st->ted[0] - yr) + st->ted[3] * (st->ted[1] - yi);
            if (hist == 1) {
                st->ted[0] = 0.f; st->ted[1] = 0.f; st->ted[2] = yr; st->ted[3] = yi;
            } else if (hist != 0) {
                st->ted[0] = st->ted[2]; st->ted[1] = st->ted[3]; st->ted[2] = yr; st->ted[3] = yi;
            }
            const float vp = e * kp;
            const float vi = st->lf_prev_in + e * ki;
            st->lf_prev_in = vi;
            st->lf_output = vp + vi;
            const float W = st->lf_output + 0.5f;
            st->prev_is_strobe = st->is_strobe;
            st->is_strobe = st->nco < W ? 1 : 0;
            if (st->is_strobe == 1) {
                st->mu = st->nco / W;
                farrow_taps(st->mu, b);
                st->nco += 1.0f;
            }
            st->nco = st->nco - W;
            /* the PLL */
            int cut = 0;
            if (strobe == 1) {
                const int k0 = c->nu_k;
                update_phase(c, st->last[0], st->last[1], P, n_p, pl_frame, pg, ig, sps);
                cut = c->nu_k != k0;
            }
            if (--to_frame_end == 0) {
                MU[frame] = st->mu;
                FRQ[frame] = c->est;
                PHS[frame] = 0.f;
                frame++;
                to_frame_end = N;
            }
            if (cut) {                                                         /* what lies behind sample i was rotated with the old nu */
                if (n_cuts < max_cuts) { cuts[2 * n_cuts] = (int)k; cuts[2 * n_cuts + 1] = i; }
                n_cuts++;
                fin = i + 1;
                break;
            }
        }
        memmove(zb, zb + 2 * fin, sizeof(float) * 2 * (MF_T - 1));             /* the window moves on by the final samples */
        c->n = (c->n + fin) % NCO_TURN_UNITS;
        t += fin;
    }
    memcpy(ring, zb, sizeof(float) * 2 * (MF_T - 1));
    return n_cuts;
}
