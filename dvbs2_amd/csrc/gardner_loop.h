// The Gardner timing loop at two samples per symbol, stated once for the kernels that run it: stm_sync_kernel (k_timing.hip), stepmf_kernel (k_stepmf.hip) and
// stm_ultra_kernel (k_timing_ultra.hip).  Per complex input sample x, with one stream's state in registers (GardnerRegs):
//   the Farrow step : the 4-tap piecewise-parabolic interpolator (Filter_Farrow_ccr_naive.hxx, set_mu / step)
//                         b0 = mu^2/2 - mu/2,  b1 = 1 - mu/2 - mu^2/2,  b2 = mu + mu/2 - mu^2/2,  b3 = b0;   y = (b0 x[n-3] + b1 x[n-2]) + (b2 x[n-1] + b3 x[n])
//   the detector    : with h = is_strobe + 2 prev_is_strobe (the strobe history) and the TED buffer {T0, T1}: on h == 1 Gardner's error e = T1 . (T0 - y); y enters the buffer
//   the loop filter : PI: lf_prev_in += e ki, lf_output = lf_prev_in + e kp
//   the control     : W = lf_output + 1/2, prev_is_strobe = is_strobe, is_strobe = NCO < W; a strobe sets mu = NCO / W (correctly rounded; the taps follow) and moves the NCO
//                     by 1 - W, anything else by -W
// The chain from one sample to the next is NCO compare -> mu -> taps -> Farrow -> detector -> filter -> W: sample-serial within a stream.
//
// The reference states detector, filter and control three times, and the three differ; each kernel follows its own, bit for bit (the C twins under tests/ are the contract):
//                                                        TED buffer, history 1 / 2 / 3     loop filter off history 1    NCO on a strobe    B         last_symbol
//   gardner_synchronize  Synchronizer_Gardner_fast_osf2::_synchronize   shift / shift / T0 = 0     skipped: lf_output = lf_prev_in    NCO + (1 - W)    h odd     kept
//   gardner_step         Synchronizer_Gardner_fast_osf2::step           T0 = 0 / shift / shift     evaluated with e = 0         (NCO + 1) - W    is_strobe     kept
//   gardner_ultra        Synchronizer_Gardner_ultra_osf2 (control)      shift / shift / T0 = 0     evaluated with e = 0         (NCO + 1) - W    is_strobe     not kept
// History 0 (skipping) leaves the buffer alone in all three.  They are three functions on purpose: `x + 0 * k` is not `x` for every x (signed zeros, NaN), and
// NCO + (1 - W) and (NCO + 1) - W round differently, so no flag merges them bit for bit.
// Every translation unit is compiled with -ffp-contract=off: no product here is fused into a sum.
#pragma once
#include "dvbs2hip_internal.h"

namespace dvbs2 {

// Filter_Farrow_ccr_naive::set_mu (b3 = b0)
__host__ __device__ __forceinline__ void farrow_taps(float mu, float &b0, float &b1, float &b2)
{
    const float half_mu = 0.5f * mu;
    const float half_mu_square = half_mu * mu;
    b0 = half_mu_square - half_mu;
    b1 = 1.0f - half_mu - half_mu_square;
    b2 = mu + half_mu - half_mu_square;
}

// Filter_Farrow_ccr_naive::step's sum over x[n-3] .. x[n], in its association (the held samples of stm_ultra_kernel keep this expression written out: see there)
__host__ __device__ __forceinline__ float farrow_sum(float b0, float b1, float b2, float x3, float x2, float x1, float x0)
{
    return (b0 * x3 + b1 * x2) + (b2 * x1 + b0 * x0);
}

// one stream's StmState in registers, and the taps of its mu
struct GardnerRegs {
    float h1r, h1i, h2r, h2i, h3r, h3i;          // the Farrow history x[n-1], x[n-2], x[n-3]
    float t0r, t0i, t1r, t1i;                    // the TED buffer {T0, T1}
    float mu, nco, lfp, lfo, lsr, lsi;           // lf_prev_in, lf_output, last_symbol
    int is, prev;                                // is_strobe, prev_is_strobe
    float b0, b1, b2;

    __device__ __forceinline__ void load(const StmState &st)
    {
        h1r = st.h[0]; h1i = st.h[1]; h2r = st.h[2]; h2i = st.h[3]; h3r = st.h[4]; h3i = st.h[5];
        t0r = st.ted[0]; t0i = st.ted[1]; t1r = st.ted[2]; t1i = st.ted[3];
        mu = st.mu; nco = st.nco; lfp = st.lf_prev_in; lfo = st.lf_output; lsr = st.last[0]; lsi = st.last[1];
        is = st.is_strobe; prev = st.prev_is_strobe;
        farrow_taps(mu, b0, b1, b2);
    }

    __device__ __forceinline__ void store(StmState &st) const
    {
        st.h[0] = h1r; st.h[1] = h1i; st.h[2] = h2r; st.h[3] = h2i; st.h[4] = h3r; st.h[5] = h3i;
        st.ted[0] = t0r; st.ted[1] = t0i; st.ted[2] = t1r; st.ted[3] = t1i;
        st.mu = mu; st.nco = nco; st.lf_prev_in = lfp; st.lf_output = lfo; st.last[0] = lsr; st.last[1] = lsi;
        st.is_strobe = is; st.prev_is_strobe = prev;
    }

    // the Farrow step: the output for the input sample x, which enters the history
    __device__ __forceinline__ void farrow(float xr, float xi, float &yr, float &yi)
    {
        yr = farrow_sum(b0, b1, b2, h3r, h2r, h1r, xr);
        yi = farrow_sum(b0, b1, b2, h3i, h2i, h1i, xi);
        h3r = h2r; h3i = h2i; h2r = h1r; h2i = h1i; h1r = xr; h1i = xi;
    }

    __device__ __forceinline__ float ted_error(float yr, float yi) const { return t1r * (t0r - yr) + t1i * (t0i - yi); }
    __device__ __forceinline__ void ted_shift(float yr, float yi) { t0r = t1r; t0i = t1i; t1r = yr; t1i = yi; }
    __device__ __forceinline__ void ted_restart(float yr, float yi) { t0r = 0.f; t0i = 0.f; t1r = yr; t1i = yi; }

    // the loop filter as step() and ULTRA write it (loop_filter, Synchronizer_Gardner_fast_osf2.hxx:23-35)
    __device__ __forceinline__ void loop_filter(float e, float kp, float ki)
    {
        const float vp = e * kp;
        const float vi = lfp + e * ki;
        lfp = vi;
        lfo = vp + vi;
    }

    // interpolation control in _synchronize's form (Synchronizer_Gardner_fast_osf2.cpp:47-164): NCO + (1 - W) on a strobe
    __device__ __forceinline__ void control_nco_plus_1mw()
    {
        const float W = lfo + 0.5f;
        prev = is;
        is = nco < W ? 1 : 0;
        if (is) {
            mu = nco / W;
            farrow_taps(mu, b0, b1, b2);
            nco = nco + (1.0f - W);
        } else {
            nco = nco - W;
        }
    }

    // interpolation control in the form of step() and of ULTRA (interpolation_control, .hxx:37-53 and ultra .hxx:102-120): (NCO + 1) - W on a strobe.
    // The taps are the caller's: step() sets them on a strobe, ULTRA after every sample (mu is unchanged off a strobe, so the values agree).
    __device__ __forceinline__ void control_nco1_minus_w()
    {
        const float W = lfo + 0.5f;
        prev = is;
        is = nco < W ? 1 : 0;
        if (is) {
            mu = nco / W;
            nco = nco + 1.0f;
        }
        nco = nco - W;
    }
};

// Each of the three takes the Farrow output y of the sample, moves detector, loop filter and interpolation control past it, and returns the sample's B.

// Synchronizer_Gardner_fast_osf2::_synchronize (Synchronizer_Gardner_fast_osf2.cpp:35-166).  Alone in skipping the loop filter off history 1 and in NCO + (1 - W).
__device__ __forceinline__ int gardner_synchronize(GardnerRegs &g, float yr, float yi, float kp, float ki)
{
    const int hist = g.is + 2 * g.prev;
    if (hist == 1) {
        const float e = g.ted_error(yr, yi);
        g.lfp = g.lfp + e * ki;
        g.lfo = g.lfp + e * kp;
        g.ted_shift(yr, yi);
    } else {
        g.lfo = g.lfp;
        if (hist == 2) g.ted_shift(yr, yi);
        else if (hist == 3) g.ted_restart(yr, yi);
    }
    const int strobe = hist & 1;
    if (strobe) { g.lsr = yr; g.lsi = yi; }
    g.control_nco_plus_1mw();
    return strobe;
}

// Synchronizer_Gardner_fast_osf2::step (Synchronizer_Gardner_fast_osf2.hxx:8-87), what Synchronizer_step_mf_cc calls.  Alone in TED_update's cases: history 1 restarts
// the buffer where the other two shift, history 3 shifts where they restart.
__device__ __forceinline__ int gardner_step(GardnerRegs &g, float yr, float yi, float kp, float ki)
{
    const int strobe = g.is;
    if (strobe) { g.lsr = yr; g.lsi = yi; }
    const int hist = g.is + 2 * g.prev;
    float e = 0.0f;
    if (hist == 1) {
        e = g.ted_error(yr, yi);
        g.ted_restart(yr, yi);
    } else if (hist != 0) {
        g.ted_shift(yr, yi);
    }
    g.loop_filter(e, kp, ki);
    g.control_nco1_minus_w();
    if (g.is) farrow_taps(g.mu, g.b0, g.b1, g.b2);
    return strobe;
}

// A control sample of Synchronizer_Gardner_ultra_osf2 (TED_update, loop_filter, interpolation_control: Synchronizer_Gardner_ultra_osf2.hxx:58-120).  _synchronize's
// buffer cases with step()'s filter and NCO; alone in not keeping last_symbol and in setting the taps after every sample.
__device__ __forceinline__ int gardner_ultra(GardnerRegs &g, float yr, float yi, float kp, float ki)
{
    const int strobe = g.is;
    const int hist = 2 * g.prev + g.is;
    float e = 0.0f;
    if (hist == 1) e = g.ted_error(yr, yi);
    if (hist == 1 || hist == 2) g.ted_shift(yr, yi);
    else if (hist == 3) g.ted_restart(yr, yi);
    g.loop_filter(e, kp, ki);
    g.control_nco1_minus_w();
    farrow_taps(g.mu, g.b0, g.b1, g.b2);
    return strobe;
}

}  // namespace dvbs2
