/*
 * timing_ultra_twin.c -- CPU twin of the held Gardner loop (the reference's `--stm-type ULTRA`, Synchronizer_Gardner_ultra_osf2).  TEST INFRASTRUCTURE ONLY:
 * tests/timing_ultra_ref.py compiles it with the system compiler (-O2 -ffp-contract=off, so that no product is fused into a sum) and loads it with ctypes; the GPU tests hold
 * libdvbs2hip's stm_ultra_kernel to it bit for bit.  Written from the algorithm, one stream at a time, sample by sample in the reference's order.
 * Citations are relative to the reference's src/common/Module/Synchronizer/Synchronizer_timing/.
 *
 * Once the loop is locked (`act`), every frame of N complex samples is cut into N / H hold blocks of H samples (H = the hold size) and a tail of N mod H samples; the blocks start
 * over at every frame.  Over the first H - 4 samples of a block the loop HOLDS: mu and the Farrow taps stay, the strobe alternates, the NCO moves by +-1/2 and only the
 * detector and the loop filter run.  The last four samples of a block and the tail are CONTROL samples: the whole loop, interpolation control included.  With `act` clear every
 * sample is a control sample.  (Synchronizer_Gardner_ultra_osf2.cpp:59-133.)
 */
#include <string.h>
#include "gardner_twin.h"

/* set_loop_filter_coeffs, .cpp:341-351: the same formula as FAST */
void twin_ultra_gains(float damping, float nbw, float dg, float *kp, float *ki) { loop_gains(damping, nbw, dg, kp, ki); }

/* TED_update (.hxx:58-87) then loop_filter (.hxx:89-100); returns the strobe history of the sample */
static int detector_and_filter(twin_stm *st, float yr, float yi, float kp, float ki)
{
    const int old = st->prev_is_strobe, is = st->is_strobe;
    const int hist = old * 2 + is;
    st->prev_is_strobe = is;
    float e = 0.0f;
    if (hist == 1) e = st->ted[2] * (st->ted[0] - yr) + st->ted[3] * (st->ted[1] - yi);
    if ((old ^ is) == 1) {                           /* histories 1 and 2: shift */
        st->ted[0] = st->ted[2]; st->ted[1] = st->ted[3]; st->ted[2] = yr; st->ted[3] = yi;
    } else if ((old & is) == 1) {                    /* history 3, stuffing */
        st->ted[0] = 0.f; st->ted[1] = 0.f; st->ted[2] = yr; st->ted[3] = yi;
    }                                                /* history 0, skipping: nothing */
    const float vp = e * kp;
    const float vi = st->lf_prev_in + e * ki;
    st->lf_prev_in = vi;
    st->lf_output = vp + vi;
    return hist;
}

/* interpolation_control (.hxx:102-120) and the set_mu behind it */
static void interpolation_control(twin_stm *st, float b[3])
{
    const float W = st->lf_output + 0.5f;
    st->is_strobe = st->nco < W ? 1 : 0;
    if (st->is_strobe) {
        st->mu = st->nco / W;
        st->nco = st->nco + 1.0f;
    }
    st->nco = st->nco - W;
    farrow_taps(st->mu, b);
}

static void control_sample(twin_stm *st, float b[3], const float *X, float *Y, int *B, long long k, float kp, float ki)
{
    float yr, yi;
    farrow(st, b, X[2 * k], X[2 * k + 1], &yr, &yi);
    Y[2 * k] = yr; Y[2 * k + 1] = yi;
    B[2 * k] = st->is_strobe; B[2 * k + 1] = st->is_strobe;
    detector_and_filter(st, yr, yi, kp, ki);
    interpolation_control(st, b);
}

/* Synchronizer_timing::synchronize (Synchronizer_timing.hxx:189-201) over n_frames frames of N complex samples of ONE stream, each frame
 * Synchronizer_Gardner_ultra_osf2::_synchronize (.cpp:59-133) with hold size H and the flag `act`.
 * first_hist (may be NULL): the strobe history of every hold block's first held sample, n_frames * (N / H) entries -- the trace the tests' coverage condition reads. */
void twin_ultra_synchronize(twin_stm *st, const float *X, float *Y, int *B, float *MU, int n_frames, int N, int H, int act, float kp, float ki, int *first_hist)
{
    float b[3];
    farrow_taps(st->mu, b);
    const int hold_nbr = act ? N / H : 0;
    for (int f = 0; f < n_frames; f++) {
        const long long base = (long long)f * N;
        for (int blk = 0; blk < hold_nbr; blk++) {
            const long long i = base + (long long)blk * H;
            /* the held samples: the Farrow filter with the taps in force over the block, B alternating from is_strobe ... */
            for (int j = 0; j < H - 4; j++) {
                float yr, yi;
                farrow(st, b, X[2 * (i + j)], X[2 * (i + j) + 1], &yr, &yi);
                Y[2 * (i + j)] = yr; Y[2 * (i + j) + 1] = yi;
            }
            int p = st->is_strobe;
            for (int j = 0; j < H - 4; j++) { B[2 * (i + j)] = p; B[2 * (i + j) + 1] = p; p = 1 - p; }
            /* ... then detector and loop filter per sample, the strobe toggling, the NCO moving by is_strobe - 1/2 */
            for (int j = 0; j < H - 4; j++) {
                const int hist = detector_and_filter(st, Y[2 * (i + j)], Y[2 * (i + j) + 1], kp, ki);
                if (j == 0 && first_hist) first_hist[(long long)f * hold_nbr + blk] = hist;
                st->is_strobe = 1 - st->is_strobe;
                st->nco = st->nco + ((float)st->is_strobe - 0.5f);
            }
            for (int j = H - 4; j < H; j++) control_sample(st, b, X, Y, B, i + j, kp, ki);
        }
        for (long long k = base + (long long)hold_nbr * H; k < base + N; k++) control_sample(st, b, X, Y, B, k, kp, ki);
        MU[f] = st->mu;
    }
}
