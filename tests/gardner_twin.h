/*
 * gardner_twin.h -- what the three CPU twins of the timing loop share (timing_twin.c, timing_ultra_twin.c, stepmf_twin.c).  TEST INFRASTRUCTURE ONLY, and written from
 * the algorithm like the twins: it includes nothing of the library's, so that the twins stay a second statement of the arithmetic.  What differs between the three loops --
 * detector, loop filter, interpolation control -- is not here but in each twin, next to its citations.  Citations are relative to the reference's src/common/Module/.
 */
#ifndef GARDNER_TWIN_H
#define GARDNER_TWIN_H

/* one stream's state, the layout of the library's StmState; all zeros = reset (Synchronizer_timing::reset, Synchronizer_timing.hxx:96-111, with
 * Synchronizer_Gardner_fast_osf2::_reset, .cpp:168-186, or Synchronizer_Gardner_ultra_osf2::_reset, .cpp:322-339) */
typedef struct {
    float h[6];           /* Farrow history x[n-1], x[n-2], x[n-3] (re, im) */
    float ted[4];         /* TED_buffer[0], TED_buffer[1] (re, im) */
    float mu, nco, lf_prev_in, lf_output;
    float last[2];        /* last_symbol (ULTRA's _synchronize does not maintain it) */
    int is_strobe, prev_is_strobe;      /* prev_is_strobe: the is_strobe the detector saw last, the low bit of ULTRA's strobe_history */
} twin_stm;

/* Filter_Farrow_ccr_naive::set_mu, Filter/Filter_FIR/Farrow/Filter_Farrow_ccr_naive.hxx (b[3] = b[0]) */
static inline void farrow_taps(float mu, float b[3])
{
    float half_mu = 0.5f * mu;
    float half_mu_square = half_mu * mu;
    b[0] = half_mu_square - half_mu;
    b[1] = 1.0f - half_mu - half_mu_square;
    b[2] = mu + half_mu - half_mu_square;
}

/* one Farrow output: Filter_Farrow_ccr_naive::step, and Filter_FIR_ccr::_filter with four taps (Filter/Filter_FIR/Filter_FIR_ccr.cpp:68-142), which sums in the same order */
static inline void farrow(twin_stm *st, const float b[3], float xr, float xi, float *yr, float *yi)
{
    const float r0 = st->h[4] * b[0], i0 = st->h[5] * b[0];
    const float r1 = st->h[2] * b[1], i1 = st->h[3] * b[1];
    const float r2 = st->h[0] * b[2], i2 = st->h[1] * b[2];
    const float r3 = xr * b[0], i3 = xi * b[0];
    *yr = (r0 + r1) + (r2 + r3);
    *yi = (i0 + i1) + (i2 + i3);
    st->h[4] = st->h[2]; st->h[5] = st->h[3]; st->h[2] = st->h[0]; st->h[3] = st->h[1]; st->h[0] = xr; st->h[1] = xi;
}

/* set_loop_filter_coeffs: Synchronizer_Gardner_fast_osf2.cpp:188-198 and, the same formula, Synchronizer_Gardner_ultra_osf2.cpp:341-351 (in float, as the reference's
 * R = float build evaluates it) */
static inline void loop_gains(float damping, float nbw, float dg, float *kp, float *ki)
{
    float K0 = -1.f;
    float theta = nbw / 2.0f / (damping + 0.25f / damping);
    float d = (1.f + 2.f * damping * theta + theta * theta) * K0 * dg;
    *kp = (4.f * damping * theta) / d;
    *ki = (4.f * theta * theta) / d;
}

#endif
