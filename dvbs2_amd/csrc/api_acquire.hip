// C ABI, acquisition: symbol timing (stm_*), coarse frequency and the step_mf loop (sfc_*, smf_*), the channel's delay and frequency shift.
#include "dvbs2hip_handle.h"
#include "gardner_loop.h"

using namespace dvbs2;

extern "C" {

// ------------------------------------------------------------------ symbol-timing recovery (Synchronizer_Gardner_fast_osf2) and the channel's delay tasks (k_timing.hip)
// Synchronizer_Gardner_fast_osf2::set_loop_filter_coeffs, Synchronizer_Gardner_fast_osf2.cpp:188-198 (in float, as the reference's R = float build evaluates it)
static void stm_gains(float damping, float nbw, float dg, float &kp, float &ki)
{
    const float K0 = -1.f;
    const float theta = nbw / 2.0f / (damping + 0.25f / damping);
    const float d = (1.f + 2.f * damping * theta + theta * theta) * K0 * dg;
    kp = (4.f * damping * theta) / d;
    ki = (4.f * theta * theta) / d;
}

static int stm_frame_cplx(dvbs2hip_t *h) { return h->pl_frame * h->fir_osf; }        // N_in / 2: pl_frame * osf complex samples per frame (DVBS2.cpp:175)

static int stm_check(dvbs2hip_t *h, int F)
{
    int r = check_frames(h, F); if (r) return r;
    if (h->fir_osf != 2) return fail(h, DVBS2HIP_EUNSUPPORTED, "the timing synchronizer is Synchronizer_Gardner_fast_osf2: two samples per symbol only");
    if (F % h->stm.S) return fail(h, DVBS2HIP_EINVAL, "'n_frames' has to be a multiple of the stream count ('n_frames' = " + std::to_string(F) + ", streams = " + std::to_string(h->stm.S) + ").");
    // the carry buffers (4 N F/S reals per stream) and the underflow counters (one per frame slot) are laid out for one F/S: a change needs a reset first
    if (h->stm.Fs && F / h->stm.S != h->stm.Fs)
        return fail(h, DVBS2HIP_EINVAL, "'n_frames' / streams has changed since the last reset (" + std::to_string(F / h->stm.S) + " instead of " + std::to_string(h->stm.Fs) +
                                            " frames per stream): call dvbs2hip_sync_timing_reset first");
    return 0;
}

// state for S streams, all zero (= Synchronizer_timing::reset + _reset); the carry buffers are sized on the first extract
static int stm_alloc(dvbs2hip_t *h, int S)
{
    auto &T = h->stm;
    int r;
    const int n_alloc = std::max(T.n_alloc, S);                         // (streams the buffers hold once every allocation below has succeeded)
    if (T.n_alloc < S) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < 2; i++) { HIPCHK(h, dev_free(h, &T.st.p[i])); HIPCHK(h, dev_free(h, &T.ccnt.p[i])); HIPCHK(h, dev_free(h, &T.carry.p[i])); }
        T.cap = 0;
        T.n_alloc = 0;
        const char *what = "hipMalloc of the timing synchronizer's state failed";
        for (int i = 0; i < 2; i++)
            if ((r = dev_alloc(h, &T.st.p[i], sizeof(StmState) * (size_t)S, what)) || (r = dev_alloc(h, &T.ccnt.p[i], sizeof(int32_t) * (size_t)S, what))) return r;
    }
    if (!T.uf && (r = dev_alloc(h, &T.uf, sizeof(int32_t) * (size_t)h->max_frames, "hipMalloc of the timing synchronizer's underflow counters failed"))) return r;
    T.n_alloc = n_alloc;
    T.st.cur = T.carry.cur = T.ccnt.cur = 0;
    T.Fs = 0;
    HIPCHK(h, hipMemsetAsync(T.st.in(), 0, sizeof(StmState) * (size_t)S, h->stream));
    HIPCHK(h, hipMemsetAsync(T.ccnt.in(), 0, sizeof(int32_t) * (size_t)S, h->stream));
    HIPCHK(h, hipMemsetAsync(T.uf, 0, sizeof(int32_t) * (size_t)h->max_frames, h->stream));
    return 0;
}

// what every device form does first: the streams' state on first use, frames per stream, the loop gains
static int stm_begin(dvbs2hip_t *h, int F, const char *task)
{
    auto &T = h->stm;
    if (T.n_alloc < T.S) {
        if (h->capturing) return fail(h, DVBS2HIP_EINVAL, std::string("run the sequence once before recording it: the first ") + task + " allocates the streams' state");
        if (int r = stm_alloc(h, T.S)) return r;
    }
    T.Fs = F / T.S;
    if (T.kp == 0.f) stm_gains(T.damping, T.nbw, T.dg, T.kp, T.ki);
    return 0;
}

// carry buffers of at least `cap` reals per stream; what the old ones held moves over (a strided copy)
static int stm_carry(dvbs2hip_t *h, long long cap)
{
    auto &T = h->stm;
    if (T.cap >= cap) return 0;
    float *nb[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; i++)      // both buffers or neither
        if (int r = dev_alloc(h, &nb[i], sizeof(float) * (size_t)cap * (size_t)T.n_alloc, "hipMalloc of the timing synchronizer's carry buffers failed")) { (void)dev_free(h, &nb[0]); return r; }
    if (T.cap > 0) {
        HIPCHK(h, hipMemcpy2DAsync(nb[T.carry.cur], sizeof(float) * (size_t)cap, T.carry.in(), sizeof(float) * (size_t)T.cap, sizeof(float) * (size_t)T.cap, (size_t)T.n_alloc,
                                   hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    for (int i = 0; i < 2; i++) { HIPCHK(h, dev_free(h, &T.carry.p[i])); T.carry.p[i] = nb[i]; }
    T.cap = cap;
    return 0;
}

int dvbs2hip_sync_timing_set_params(dvbs2hip_t *h, float damping, float nbw, float detector_gain)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (!(damping > 0.f) || !(nbw > 0.f) || !(detector_gain > 0.f) || !std::isfinite(damping) || !std::isfinite(nbw) || !std::isfinite(detector_gain))
        return fail(h, DVBS2HIP_EINVAL, "'damping', 'nbw' and 'detector_gain' have to be positive");
    h->stm.damping = damping; h->stm.nbw = nbw; h->stm.dg = detector_gain;
    stm_gains(damping, nbw, detector_gain, h->stm.kp, h->stm.ki);
    return 0;
}

int dvbs2hip_sync_timing_get_gains(dvbs2hip_t *h, float *proportional, float *integrator)
{
    if (!h || !proportional || !integrator) return DVBS2HIP_EINVAL;
    stm_gains(h->stm.damping, h->stm.nbw, h->stm.dg, *proportional, *integrator);
    return 0;
}

int dvbs2hip_sync_timing_set_streams(dvbs2hip_t *h, int32_t S)
{
    int r0 = enter(h); if (r0) return r0;
    if (S < 1 || S > h->max_frames) return fail(h, DVBS2HIP_EINVAL, "'S' has to be in [1, max_frames] ('S' = " + std::to_string(S) + ").");
    if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "a capture is open on this handle");
    h->stm.S = S;
    return stm_alloc(h, S);
}

int dvbs2hip_sync_timing_reset(dvbs2hip_t *h)
{
    int r0 = enter(h); if (r0) return r0;
    if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "a capture is open on this handle");
    h->stm.act = false;                                                 // Synchronizer_timing::reset, Synchronizer_timing.hxx:109
    return stm_alloc(h, h->stm.S);
}

int dvbs2hip_sync_timing_set_type(dvbs2hip_t *h, int32_t type, int32_t hold_size)
{
    int r0 = enter(h); if (r0) return r0;
    if (type != DVBS2HIP_STM_FAST && type != DVBS2HIP_STM_ULTRA)
        return fail(h, DVBS2HIP_EINVAL, "'type' has to be DVBS2HIP_STM_FAST or DVBS2HIP_STM_ULTRA ('type' = " + std::to_string(type) + ").");
    if (type == DVBS2HIP_STM_ULTRA && hold_size <= 4)                   // Synchronizer_Gardner_ultra_osf2.cpp:27
        return fail(h, DVBS2HIP_EINVAL, "'hold_size' has to be greater than 4 ('hold_size' = " + std::to_string(hold_size) + ").");
    if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "a capture is open on this handle");
    h->stm.type = type;
    if (type == DVBS2HIP_STM_ULTRA) h->stm.hold = hold_size;
    h->stm.act = false;
    return stm_alloc(h, h->stm.S);
}

int dvbs2hip_sync_timing_set_act(dvbs2hip_t *h, int32_t act)
{
    int r0 = enter(h); if (r0) return r0;
    h->stm.act = act != 0;
    return 0;
}

int dvbs2hip_sync_timing_synchronize_dev(dvbs2hip_t *h, const float *X_N1, float *Y_N1, int32_t *B_N1, float *MU, int32_t F)
{
    int r = stm_check(h, F); if (r) return r;
    if (!X_N1 || !Y_N1 || !B_N1 || !MU) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    auto &T = h->stm;
    if ((r = stm_begin(h, F, "synchronize"))) return r;
    Timer tm(h, DVBS2HIP_K_MISC);
    if (T.type == DVBS2HIP_STM_ULTRA)
        HIPCHK(h, stm_ultra_launch(X_N1, Y_N1, B_N1, MU, T.st.in(), T.st.out(), T.S, F / T.S, stm_frame_cplx(h), T.hold, T.act ? 1 : 0, T.kp, T.ki, h->stream));
    else
        HIPCHK(h, stm_sync_launch(X_N1, Y_N1, B_N1, MU, T.st.in(), T.st.out(), T.S, F / T.S, stm_frame_cplx(h), T.kp, T.ki, h->stream));
    T.st.flip();
    return 0;
}

int dvbs2hip_sync_timing_synchronize(dvbs2hip_t *h, const float *X_N1, float *Y_N1, int32_t *B_N1, float *MU, int32_t F)
{
    int r = stm_check(h, F); if (r) return r;
    const size_t n4 = (size_t)F * 2 * stm_frame_cplx(h) * 4;      // floats and int32 alike
    return host_call(h, F, false, {{X_N1, B_STM_X, n4}}, {{Y_N1, B_STM_Y, n4}, {B_N1, B_STM_B, n4}, {MU, B_STM_MU, (size_t)F * sizeof(float)}}, [&](void *const *i, void *const *o, int nf) {
        return dvbs2hip_sync_timing_synchronize_dev(h, (const float *)i[0], (float *)o[0], (int32_t *)o[1], (float *)o[2], nf);
    });
}

int dvbs2hip_sync_timing_extract_dev(dvbs2hip_t *h, const float *Y_N1, const int32_t *B_N1, float *Y_N2, int32_t *UFW, int32_t *RDY, int32_t F)
{
    int r = stm_check(h, F); if (r) return r;
    if (!Y_N1 || !B_N1 || !Y_N2 || !UFW || !RDY) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    auto &T = h->stm;
    if ((r = stm_begin(h, F, "extract"))) return r;
    const int N = stm_frame_cplx(h), Fs = F / T.S;
    const long long cap = 4LL * Fs * N;                  // reals per stream: four frames' worth of output per frame of the call
    if (T.cap < cap) {
        if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "run the sequence once before recording it: the first extract of this size allocates");
        if ((r = stm_carry(h, cap))) return r;
    }
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, stm_extract_launch(Y_N1, B_N1, Y_N2, UFW, RDY, T.carry.in(), T.ccnt.in(), T.carry.out(), T.ccnt.out(), T.uf, T.S, Fs, N, T.cap, h->stream));
    T.carry.flip(), T.ccnt.flip();
    return 0;
}

int dvbs2hip_sync_timing_extract(dvbs2hip_t *h, const float *Y_N1, const int32_t *B_N1, float *Y_N2, int32_t *UFW, int32_t *RDY, int32_t F)
{
    int r = stm_check(h, F); if (r) return r;
    const size_t n4 = (size_t)F * 2 * stm_frame_cplx(h) * 4;
    const HostSock y2 = {Y_N2, B_STM_Y2, n4 / 2};      // in and out: the frames of a stream that is not ready keep what the socket held past the symbols written
    return host_call(h, F, false, {{Y_N1, B_STM_Y, n4}, {B_N1, B_STM_B, n4}, y2}, {y2, {UFW, B_STM_UFW, (size_t)F * sizeof(int32_t)}, {RDY, B_STM_RDY, (size_t)h->stm.S * sizeof(int32_t)}},
                     [&](void *const *i, void *const *o, int nf) {
        return dvbs2hip_sync_timing_extract_dev(h, (const float *)i[0], (const int32_t *)i[1], (float *)o[0], (int32_t *)o[1], (int32_t *)o[2], nf);
    });
}

int dvbs2hip_channel_set_delay(dvbs2hip_t *h, float D)
{
    int r0 = enter(h); if (r0) return r0;
    if (!(D >= 2.f) || !(D <= 16777216.f)) return fail(h, DVBS2HIP_EINVAL, "Argument 'max_delay' has to be greater than 2.");     // DVBS2.cpp:129-133 (and at most 2^24 samples here)
    if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "a capture is open on this handle");
    auto &C = h->chn;
    farrow_taps(D - floorf(D), C.b[0], C.b[1], C.b[2]);                 // mu: DVBS2.cpp:522
    const long long H = (long long)floorf(D) + 1;                       // (floor(D) - 2) samples of delay line + 3 of the Farrow filter
    if (H > C.H || !C.hist.p[0]) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < 2; i++) {
            HIPCHK(h, dev_free(h, &C.hist.p[i]));
            if (int r = dev_alloc(h, &C.hist.p[i], sizeof(float) * 2 * (size_t)H, "hipMalloc of the channel delay's history failed")) return r;
        }
    }
    C.D = D; C.H = H; C.hist.cur = 0;
    HIPCHK(h, hipMemsetAsync(C.hist.in(), 0, sizeof(float) * 2 * (size_t)H, h->stream));
    return 0;
}

int dvbs2hip_channel_delay_dev(dvbs2hip_t *h, const float *X, float *Y, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X || !Y) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    auto &C = h->chn;
    if (!C.hist.p[0] && (r = dvbs2hip_channel_set_delay(h, C.D))) return r;
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, chn_delay_launch(X, Y, C.hist.in(), C.hist.out(), C.H, (long long)F * stm_frame_cplx(h), C.b[0], C.b[1], C.b[2], h->stream));
    C.hist.flip();
    return 0;
}

int dvbs2hip_channel_delay(dvbs2hip_t *h, const float *X, float *Y, int32_t F)
{
    const size_t n = h ? (size_t)2 * stm_frame_cplx(h) : 0;
    return host_wrap(h, X, n, Y, n, F, [&](const float *a, float *b, int nf) { return dvbs2hip_channel_delay_dev(h, a, b, nf); });
}

// ------------------------------------------------------------------ Synchronizer_freq_coarse: the frequency shift of the transmission phase (block-wise) and the loop that finds it (k_stepmf.hip)
static void sfc_state_reset(dvbs2hip_t *h, SfcState &c)                // Synchronizer_freq_coarse::reset + Synchronizer_freq_coarse_DVBS2_aib::_reset, .cpp:115-129; last_delay is Synchronizer_step_mf_cc's and stays
{
    const int32_t last_delay = c.last_delay;
    c = SfcState{};
    c.curr_idx = h->pl_frame - 1;
    c.last_delay = last_delay;
}

// the host copy of the streams' states, current
static int sfc_host(dvbs2hip_t *h)
{
    auto &C = h->sfc;
    const size_t S = (size_t)h->stm.S;
    if (C.hs.size() != S) {                                            // a new stream count: every stream starts over
        C.hs.assign(S, SfcState{});
        for (auto &c : C.hs) sfc_state_reset(h, c);
        C.frq.assign(S, 0.f);
        C.where = C.HOST;
        C.hist_stale = true;
    }
    if (C.where == C.DEV) {
        if (h->capturing) return fail(h, DVBS2HIP_EUNSUPPORTED, "the coarse synchronizer's state has to come back from the device: not inside a capture");
        HIPCHK(h, hipMemcpyAsync(C.hs.data(), C.cf.in(), sizeof(SfcState) * S, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (size_t s = 0; s < S; s++) C.frq[s] = C.hs[s].est;         // after the loop FRQ is estimated_freq (Synchronizer_freq_coarse.hxx:121-124)
        C.where = C.BOTH;
    }
    return 0;
}

// Synchronizer_freq_coarse_DVBS2_aib::set_PLL_coeffs, .cpp:94-113, R = float (the 0.25 there is a double constant: the quotient is rounded to float once)
static void sfc_gains(int pll_sps, float damping, float nbw, float &pg, float &ig)
{
    const float det_gain = 2.0f;
    const float bw = nbw * (float)pll_sps;
    const float K0 = (float)pll_sps;
    const float theta = (float)((double)bw / (((double)damping + 0.25 / (double)damping) * (double)(float)pll_sps));
    const float d = 1.0f + 2.0f * damping * theta + theta * theta;
    pg = (4.0f * damping * theta / d) / (det_gain * K0);
    ig = (4.0f / (float)pll_sps * theta * theta / d) / (det_gain * K0);
}

int dvbs2hip_sync_coarse_set_pll(dvbs2hip_t *h, int32_t pll_sps, float damping, float nbw)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (pll_sps < 1 || !(damping > 0.f) || !(nbw > 0.f) || !std::isfinite(damping) || !std::isfinite(nbw))
        return fail(h, DVBS2HIP_EINVAL, "'pll_sps', 'damping' and 'nbw' have to be positive");
    h->sfc.pll_sps = pll_sps; h->sfc.damping = damping; h->sfc.nbw = nbw;
    return 0;
}

int dvbs2hip_sync_coarse_get_gains(dvbs2hip_t *h, float *proportional, float *integrator)
{
    if (!h || !proportional || !integrator) return DVBS2HIP_EINVAL;
    sfc_gains(h->sfc.pll_sps, h->sfc.damping, h->sfc.nbw, *proportional, *integrator);
    return 0;
}

int dvbs2hip_sync_coarse_get_freq(dvbs2hip_t *h, float *estimated_freq, float *nu)
{
    int r0 = enter(h); if (r0) return r0;
    if (!estimated_freq || !nu) return fail(h, DVBS2HIP_EINVAL, "null pointer");
    int r = sfc_host(h); if (r) return r;
    for (size_t s = 0; s < h->sfc.hs.size(); s++) { estimated_freq[s] = h->sfc.hs[s].est; nu[s] = (float)h->sfc.hs[s].nu_k / 1e6f; }
    return 0;
}

int dvbs2hip_sync_coarse_set_freq(dvbs2hip_t *h, float estimated_freq)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (!(estimated_freq == estimated_freq) || fabsf(estimated_freq) > 0.5f) return fail(h, DVBS2HIP_EINVAL, "'estimated_freq' has to be a normalized frequency in [-0.5, 0.5]");
    int r;
    if ((r = enter(h)) || (r = sfc_host(h))) return r;
    const float nu = -estimated_freq;                                  // Synchronizer_freq_coarse_DVBS2_aib.cpp:82: mult.set_nu(-estimated_freq)
    const float fk = floorf(nu * 1e6f);                                // Multiplier_sine_ccc_naive::set_nu, .cpp:44-51: new_nu = floor(nu 1e6) / 1e6
    for (size_t s = 0; s < h->sfc.hs.size(); s++) { h->sfc.hs[s].nu_k = (int32_t)fk; h->sfc.frq[s] = -(fk / 1e6f); }
    h->sfc.where = h->sfc.HOST;
    return 0;
}
int dvbs2hip_sync_coarse_reset(dvbs2hip_t *h)                          // Synchronizer_freq_coarse_DVBS2_aib::_reset, .cpp:115-129
{
    int r;
    if ((r = enter(h)) || (r = sfc_host(h))) return r;
    for (size_t s = 0; s < h->sfc.hs.size(); s++) { sfc_state_reset(h, h->sfc.hs[s]); h->sfc.frq[s] = 0.f; }
    h->sfc.where = h->sfc.HOST;
    return 0;
}
int dvbs2hip_sync_coarse_synchronize_dev(dvbs2hip_t *h, const float *X, float *FRQ, float *PHS, float *Y, int32_t n_cplx, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X || !Y) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if (n_cplx < 1) return fail(h, DVBS2HIP_EINVAL, "'n_cplx' has to be greater than 0");
    if (h->capturing) return fail(h, DVBS2HIP_EUNSUPPORTED, "the stream position is a launch argument: this task cannot be recorded into a graph");
    if ((r = sfc_host(h))) return r;
    const int S = (int)h->sfc.hs.size();
    if (F % S) return fail(h, DVBS2HIP_EINVAL, "'n_frames' has to be a multiple of the stream count ('n_frames' = " + std::to_string(F) + ", streams = " + std::to_string(S) + ").");
    Timer tm(h, DVBS2HIP_K_MISC);
    const int Fs = F / S;
    const long long total = (long long)n_cplx * Fs;
    for (int s = 0; s < S; s++) {                                      // stream s = frames [s F/S, (s+1) F/S), each with its own frequency and sample counter
        SfcState &c = h->sfc.hs[s];
        const float new_nu = (float)c.nu_k / 1e6f;
        const float omega = (float)(2 * 3.1415926535897932384626433832795 * new_nu);
        HIPCHK(h, nco_launch(X + (size_t)2 * total * s, Y + (size_t)2 * total * s, omega, (uint32_t)c.n, total, FRQ ? FRQ + (size_t)s * Fs : nullptr, PHS ? PHS + (size_t)s * Fs : nullptr,
                             h->sfc.frq[s], Fs, h->stream));
        c.n = (int32_t)(((unsigned long long)c.n + (unsigned long long)total) % 1000000ull);
    }
    h->sfc.where = h->sfc.HOST;
    return 0;
}
int dvbs2hip_sync_coarse_synchronize(dvbs2hip_t *h, const float *X, float *FRQ, float *PHS, float *Y, int32_t n_cplx, int32_t F)
{
    const size_t nb = (size_t)F * 2 * (n_cplx > 0 ? n_cplx : 0) * sizeof(float);
    // several streams: the whole call at once, on the timing tasks' buffers (a chunk of a pinned socket would cut across the streams); one stream: chunks advance the sample counter in order
    const int S = h ? h->stm.S : 1;
    int r = host_call(h, F, S == 1, {{X, S > 1 ? B_STM_X : B_IN, nb}}, {{Y, S > 1 ? B_STM_Y : B_OUT, nb}},
                      [&](void *const *i, void *const *o, int nf) { return dvbs2hip_sync_coarse_synchronize_dev(h, (const float *)i[0], nullptr, nullptr, (float *)o[0], n_cplx, nf); });
    if (r) return r;
    for (int f = 0; f < F; f++) { if (FRQ) FRQ[f] = h->sfc.frq[S > 1 ? (size_t)f / (F / S) : 0]; if (PHS) PHS[f] = 0.f; }      // FRQ / PHS are filled here: the device form got none
    return 0;
}

// the loop carries the 81-tap matched filter (smf_check): its memory is the last fir_T - 1 complex input samples per stream
constexpr int SMF_TAPS = 81;
constexpr size_t SMF_HIST_BYTES = sizeof(float) * 2 * (SMF_TAPS - 1);

// the streams' device state for the loop: allocated for S streams, current
static int sfc_dev(dvbs2hip_t *h)
{
    auto &C = h->sfc;
    const int S = h->stm.S;
    int r;
    if ((int)C.hs.size() != S || C.n_alloc < S || !C.pil || C.where == C.HOST || C.hist_stale) {
        if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "run the sequence once before recording it: the first step_mf call allocates and uploads the streams' state");
        if ((r = sfc_host(h))) return r;
    }
    if (C.n_alloc < S) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < 2; i++) { HIPCHK(h, dev_free(h, &C.cf.p[i])); HIPCHK(h, dev_free(h, &C.hist.p[i])); }
        C.n_alloc = 0;
        const char *what = "hipMalloc of the coarse synchronizer's state failed";
        for (int i = 0; i < 2; i++)
            if ((r = dev_alloc(h, &C.cf.p[i], sizeof(SfcState) * (size_t)S, what)) || (r = dev_alloc(h, &C.hist.p[i], SMF_HIST_BYTES * (size_t)S, what))) return r;
        C.hist.cur = 0;
        HIPCHK(h, hipMemsetAsync(C.hist.in(), 0, SMF_HIST_BYTES * (size_t)S, h->stream));
        C.n_alloc = S;
        C.where = C.HOST;
    }
    if (C.hist_stale) {                                                // (the buffers just allocated are clear already; older ones hold other streams' samples)
        HIPCHK(h, hipMemsetAsync(C.hist.in(), 0, SMF_HIST_BYTES * (size_t)C.n_alloc, h->stream));
        C.hist_stale = false;
    }
    if (!C.pil) {
        // scrambled_pilots, .cpp:28-31: 0 below 90, then exp(j pi/2 (R[i - 90] + 0.5)) with (R)M_PI_2 a float, the sum and std::cos / std::sin in double, rounded to float.
        // 2 pl_frame entries: set_curr_idx takes values below N_out / 2 = 2 pl_frame (Synchronizer_step_mf_cc.cpp:189); entries the reference's table does not have are 0
        std::vector<uint8_t> seq;
        pl_sequence(seq);
        const int n_p = 2 * h->pl_frame;
        std::vector<float> P(2 * (size_t)n_p, 0.f);
        const float pi_2 = 1.57079632679489661923132169163975144f;
        for (int i = 90; i < n_p && i - 90 < (int)seq.size(); i++) {
            const double a = (double)pi_2 * ((double)(float)seq[i - 90] + 0.5);
            P[2 * i] = (float)cos(a); P[2 * i + 1] = (float)sin(a);
        }
        if (upload(h, &C.pil, P)) return DVBS2HIP_EHIP;
        C.n_p = n_p;
    }
    if (C.where == C.HOST) {
        HIPCHK(h, hipMemcpyAsync(C.cf.in(), C.hs.data(), sizeof(SfcState) * (size_t)S, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));                   // (pageable source: the copy has left the host buffer before it can change)
        C.where = C.BOTH;
    }
    return 0;
}

static int smf_check(dvbs2hip_t *h, int F)
{
    int r = stm_check(h, F); if (r) return r;
    if (h->stm.type == DVBS2HIP_STM_ULTRA)
        return fail(h, DVBS2HIP_EUNSUPPORTED, "the coarse-frequency loop steps Synchronizer_Gardner_fast_osf2: with DVBS2HIP_STM_ULTRA it is not provided (dvbs2hip_sync_timing_set_type)");
    if (h->fir_T != SMF_TAPS) return fail(h, DVBS2HIP_EUNSUPPORTED, "the coarse-frequency loop carries the 81-tap matched filter: the handle's filter has another length");
    if (!h->fir_sym) return fail(h, DVBS2HIP_EUNSUPPORTED, "the coarse-frequency loop folds the matched filter over its symmetry (taps[i] == taps[80 - i]): the handle's taps are not symmetric");
    return 0;
}

int dvbs2hip_sync_step_mf_synchronize_dev(dvbs2hip_t *h, const int32_t *DEL, const float *X_N1, float *MU, float *FRQ, float *PHS, float *Y_N1, int32_t *B_N1, int32_t F)
{
    int r = smf_check(h, F); if (r) return r;
    if (!DEL || !X_N1 || !MU || !FRQ || !PHS || !Y_N1 || !B_N1) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    auto &T = h->stm;
    auto &C = h->sfc;
    const bool started_over = C.hist_stale || (int)C.hs.size() != T.S;            // (sfc_dev clears the loop's own memories then)
    if ((r = stm_begin(h, F, "synchronize")) || (r = sfc_dev(h))) return r;
    float pg, ig;
    sfc_gains(C.pll_sps, C.damping, C.nbw, pg, ig);
    // the matched filter's memory is the block-wise filter's own (the last 80 input samples per stream, oldest first) when the two stream counts agree, so dvbs2hip_filter*
    // carry on from the loop and back (bw_hist: d_hist at one stream, bw.hist at S).  Otherwise the loop keeps a memory per stream of its own, which sfc_dev has cleared
    const bool shared = h->bw.S == T.S;
    PingPong<float> *hist = &C.hist;
    if (shared) {
        if ((r = bw_hist(h, &hist))) return r;
        if (started_over && T.S > 1) HIPCHK(h, hipMemsetAsync(hist->in(), 0, SMF_HIST_BYTES * (size_t)T.S, h->stream));      // (one stream carries on from dvbs2hip_filter* whatever the loop's state)
    }
    Timer tm(h, DVBS2HIP_K_MISC);
    const auto launch = C.smf_kernel == DVBS2HIP_SMF_WAVE ? stepmf_wave_launch : stepmf_launch;      // the same arguments, state and results
    HIPCHK(h, launch(X_N1, Y_N1, B_N1, MU, FRQ, PHS, DEL, T.ccnt.in(), T.st.in(), T.st.out(), C.cf.in(), C.cf.out(), hist->in(), hist->out(), h->d_taps_rev,
                     C.pil, C.n_p, T.S, F / T.S, stm_frame_cplx(h), h->pl_frame, T.kp, T.ki, pg, ig, (float)h->fir_osf, h->stream));
    T.st.flip();
    C.cf.flip();
    hist->flip();
    C.where = C.DEV;
    return 0;
}

int dvbs2hip_sync_step_mf_synchronize(dvbs2hip_t *h, const int32_t *DEL, const float *X_N1, float *MU, float *FRQ, float *PHS, float *Y_N1, int32_t *B_N1, int32_t F)
{
    int r = smf_check(h, F); if (r) return r;
    const size_t n4 = (size_t)F * 2 * stm_frame_cplx(h) * 4, nf4 = (size_t)F * 4;
    return host_call(h, F, false, {{X_N1, B_STM_X, n4}, {DEL, B_SMF_DEL, nf4}},
                     {{Y_N1, B_STM_Y, n4}, {B_N1, B_STM_B, n4}, {MU, B_STM_MU, nf4}, {FRQ, B_SMF_FRQ, nf4}, {PHS, B_SMF_FRQ, nf4, nf4}}, [&](void *const *i, void *const *o, int nf) {
        return dvbs2hip_sync_step_mf_synchronize_dev(h, (const int32_t *)i[1], (const float *)i[0], (float *)o[2], (float *)o[3], (float *)o[4], (float *)o[0], (int32_t *)o[1], nf);
    });
}

int dvbs2hip_sync_step_mf_set_kernel(dvbs2hip_t *h, int32_t kernel)
{
    int r0 = enter(h); if (r0) return r0;
    if (kernel != DVBS2HIP_SMF_LANE && kernel != DVBS2HIP_SMF_WAVE)
        return fail(h, DVBS2HIP_EINVAL, "'kernel' has to be DVBS2HIP_SMF_LANE or DVBS2HIP_SMF_WAVE ('kernel' = " + std::to_string(kernel) + ").");
    h->sfc.smf_kernel = kernel;
    return 0;
}

int dvbs2hip_sync_step_mf_reset(dvbs2hip_t *h)                         // Synchronizer_step_mf_cc::reset, .cpp:210-217: coarse, matched filter, timing
{
    int r0 = enter(h); if (r0) return r0;
    if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "a capture is open on this handle");
    int r = dvbs2hip_sync_coarse_reset(h); if (r) return r;
    // the memory the loop runs on (dvbs2hip_sync_step_mf_synchronize_dev): the block-wise filter's when the counts agree and it exists (nothing is allocated here), else the loop's own
    PingPong<float> *hist = &h->sfc.hist;
    size_t nb = SMF_HIST_BYTES * (size_t)h->sfc.n_alloc;
    if (h->bw.S == h->stm.S && (h->bw.S == 1 || h->bw.hist_n >= h->bw.S)) { if ((r = bw_hist(h, &hist))) return r; nb = sizeof(float) * 2 * (size_t)(h->fir_T > 1 ? h->fir_T - 1 : 0) * (size_t)h->bw.S; }
    if (nb && hist->in()) HIPCHK(h, hipMemsetAsync(hist->in(), 0, nb, h->stream));
    h->stm.act = false;
    return stm_alloc(h, h->stm.S);
}

// ------------------------------------------------------------------ the channel's frequency shift: Multiplier_sine_ccc_naive built by DVBS2.cpp:624-626 from --chn-max-freq-shift, bound CH/main.cpp:63-64
int dvbs2hip_channel_set_freq_shift(dvbs2hip_t *h, float freq_shift)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (!(freq_shift == freq_shift) || fabsf(freq_shift) > 0.5f) return fail(h, DVBS2HIP_EINVAL, "'freq_shift' has to be a normalized frequency in [-0.5, 0.5]");
    const float new_nu = floorf(freq_shift / 1.0f * 1e6f) / 1e6f;       // the constructor, Multiplier_sine_ccc_naive.cpp:13-22, Fs = 1
    h->chn.fs_omega = (float)(2 * 3.1415926535897932384626433832795 * new_nu);
    h->chn.fs_n = 0;
    return 0;
}
int dvbs2hip_channel_freq_shift_dev(dvbs2hip_t *h, const float *X, float *Y, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X || !Y) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if (h->capturing) return fail(h, DVBS2HIP_EUNSUPPORTED, "the stream position is a launch argument: this task cannot be recorded into a graph");
    Timer tm(h, DVBS2HIP_K_MISC);
    const long long total = (long long)F * stm_frame_cplx(h);
    HIPCHK(h, nco_launch(X, Y, h->chn.fs_omega, h->chn.fs_n, total, nullptr, nullptr, 0.f, 0, h->stream));
    h->chn.fs_n = (uint32_t)(((unsigned long long)h->chn.fs_n + (unsigned long long)total) % 1000000ull);
    return 0;
}
int dvbs2hip_channel_freq_shift(dvbs2hip_t *h, const float *X, float *Y, int32_t F)
{
    const size_t n = h ? (size_t)2 * stm_frame_cplx(h) : 0;
    return host_wrap<true>(h, X, n, Y, n, F, [&](const float *a, float *b, int nf) { return dvbs2hip_channel_freq_shift_dev(h, a, b, nf); });
}

}  // extern "C"
