// C ABI, the pilot-aided noise estimator (k_est_pilots.hip): sigma, Eb/N0 and Es/N0 of aligned PL frames from their header and pilot symbols.  An extension with no
// reference task; beside the M2M4 estimator (dvbs2hip_estimate, dvbs2hip_api.hip), which stays the default.  Stateless unless dvbs2hip_estimate_pilots_set_alpha > 0.
#include "dvbs2hip_handle.h"
#include "rx_device.h"      // the PL frame's layout: PL_M, PL_P, PL_GAP

using namespace dvbs2;

static int estp_known(const dvbs2hip_t *h) { return PL_M + (h->pl_frame - PL_M - h->n_sym); }      // L = PL_M + PL_P N_pilots: what a PL frame holds beside its data symbols

// X_N1 with `stride` complex samples from frame to frame (compact: the L known symbols alone), or the located table SRC
static int estp_dev(dvbs2hip_t *h, const float *X_N1, const float *const *SRC, size_t stride, int compact, int32_t scrambled, float *SIG, float *EB, float *ES, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X_N1 && !SRC) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if (scrambled != 0 && scrambled != 1) return fail(h, DVBS2HIP_EINVAL, "'scrambled' has to be 0 or 1");
    const int L = estp_known(h), NS = h->bw.S;
    if (L < PL_M || L > 14 * 64) return fail(h, DVBS2HIP_EUNSUPPORTED, "the pilot-aided estimator holds at most 896 known symbols of a frame");
    const float alpha = h->estp.alpha;
    float *AN = nullptr;
    if (alpha > 0.f) {
        if (F % NS) return fail(h, DVBS2HIP_EINVAL, "'n_frames' has to be a multiple of the stream count ('n_frames' = " + std::to_string(F) + ", streams = " + std::to_string(NS) + ").");
        void *an;
        if (h->capturing && (h->estp.n_alloc < NS || h->bufs[B_ESTP_AN].bytes < 2 * sizeof(float) * (size_t)h->max_frames))
            return fail(h, DVBS2HIP_EINVAL, "run the sequence once before recording it: the first averaging call after dvbs2hip_set_streams allocates the streams' state");
        if ((r = ensure(h, B_ESTP_AN, 2 * sizeof(float) * (size_t)h->max_frames, &an))) return r;
        AN = (float *)an;
        if (h->estp.n_alloc < NS) {            // every stream's state, not started (a new stream count comes through dvbs2hip_set_streams, which has reset the old ones)
            float *st = nullptr;
            if ((r = dev_alloc(h, &st, 3 * sizeof(float) * (size_t)NS, "hipMalloc of the pilot-aided estimator's per-stream state failed"))) return r;
            if (h->estp.st) { HIPCHK(h, hipStreamSynchronize(h->stream)); (void)dev_free(h, &h->estp.st); }
            h->estp.st = st; h->estp.n_alloc = NS;
            HIPCHK(h, hipMemsetAsync(st, 0, 3 * sizeof(float) * (size_t)NS, h->stream));
        }
    }
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, est_pilots_launch(X_N1, SRC, stride, compact, h->d_plh, h->d_pl_seq, scrambled, L, h->code_rate, h->bps, AN, SIG, EB, ES, F, h->stream));
    if (AN) HIPCHK(h, est_pilots_walk_launch(AN, h->estp.st, alpha, L, h->code_rate, h->bps, SIG, EB, ES, F / NS, NS, h->stream));
    return 0;
}

extern "C" {

int dvbs2hip_estimate_pilots_dev(dvbs2hip_t *h, const float *X_N1, int32_t scrambled, float *SIG, float *EB, float *ES, int32_t F)
{
    return estp_dev(h, X_N1, nullptr, h ? (size_t)h->pl_frame : 0, 0, scrambled, SIG, EB, ES, F);
}

int dvbs2hip_estimate_pilots_located_dev(dvbs2hip_t *h, const float *const *SRC, int32_t scrambled, float *SIG, float *EB, float *ES, int32_t F)
{
    return estp_dev(h, nullptr, SRC, 0, 0, scrambled, SIG, EB, ES, F);
}

// the host form stages the known symbols of every frame and nothing else -- the header and each pilot block one strided copy over the frames: 1.3 to 7 KB of a frame of
// 27 to 266 KB
int dvbs2hip_estimate_pilots(dvbs2hip_t *h, const float *X_N1, int32_t scrambled, float *SIG, float *EB, float *ES, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X_N1) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    const int L = estp_known(h);
    if (L < PL_M) return fail(h, DVBS2HIP_EUNSUPPORTED, "the PL frame is shorter than its header and data symbols");
    const size_t cb = sizeof(float) * 2, pitch = cb * (size_t)L, fpitch = cb * (size_t)h->pl_frame, nf4 = sizeof(float) * (size_t)F;
    void *sym, *out;
    if ((r = ensure(h, B_ESTP_SYM, pitch * (size_t)F, &sym)) || (r = ensure(h, B_ESTP_OUT, 3 * nf4, &out))) return r;
    HIPCHK(h, hipMemcpy2DAsync(sym, pitch, X_N1, fpitch, cb * PL_M, (size_t)F, hipMemcpyHostToDevice, h->stream));
    for (int b = 0; b < (L - PL_M) / PL_P; b++)
        HIPCHK(h, hipMemcpy2DAsync((char *)sym + cb * (size_t)(PL_M + PL_P * b), pitch, (const char *)X_N1 + cb * (size_t)(PL_M + PL_P * b + PL_GAP * (b + 1)), fpitch, cb * PL_P, (size_t)F,
                                   hipMemcpyHostToDevice, h->stream));
    float *d_sig = (float *)out, *d_eb = d_sig + F, *d_es = d_sig + 2 * (size_t)F;
    if ((r = estp_dev(h, (const float *)sym, nullptr, (size_t)L, 1, scrambled, SIG ? d_sig : nullptr, EB ? d_eb : nullptr, ES ? d_es : nullptr, F))) return r;
    if (SIG) HIPCHK(h, hipMemcpyAsync(SIG, d_sig, nf4, hipMemcpyDeviceToHost, h->stream));
    if (EB) HIPCHK(h, hipMemcpyAsync(EB, d_eb, nf4, hipMemcpyDeviceToHost, h->stream));
    if (ES) HIPCHK(h, hipMemcpyAsync(ES, d_es, nf4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int dvbs2hip_estimate_pilots_set_alpha(dvbs2hip_t *h, float alpha)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (!(alpha >= 0.f && alpha < 1.f)) return fail(h, DVBS2HIP_EINVAL, "'alpha' has to be in [0, 1)");
    h->estp.alpha = alpha;
    return 0;
}

int dvbs2hip_estimate_pilots_reset(dvbs2hip_t *h)
{
    int r = enter(h); if (r) return r;
    if (h->estp.st) HIPCHK(h, hipMemsetAsync(h->estp.st, 0, 3 * sizeof(float) * (size_t)h->estp.n_alloc, h->stream));      // every stream's
    return 0;
}

}  // extern "C"
