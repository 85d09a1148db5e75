// C ABI, filters and what sits beside them in the sample domain: matched / shaping filter, filter1 / filter2, channel noise, decimation, the AGC stages.
#include "dvbs2hip_handle.h"

using namespace dvbs2;

extern "C" {

int dvbs2hip_set_filter_kernel(dvbs2hip_t *h, int32_t kernel)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (kernel != DVBS2HIP_FIR_AUTO && kernel != DVBS2HIP_FIR_VALU && kernel != DVBS2HIP_FIR_MFMA) return fail(h, DVBS2HIP_EINVAL, "unknown filter kernel");
    if (kernel == DVBS2HIP_FIR_MFMA && !h->d_fir_afrag) return fail(h, DVBS2HIP_EUNSUPPORTED, "the matrix-core filter takes at most 81 taps");
    h->fir_kernel = kernel;
    return 0;
}

}  // extern "C"

// the block-wise matched filter's memory for the handle's bw.S streams: d_hist at S = 1 (a part of d_hist_all), a pair of its own at S > 1 -- allocated and cleared on
// first use, both buffers or neither; a failure leaves what the handle had
int dvbs2::bw_hist(dvbs2hip_t *h, PingPong<float> **hist)
{
    auto &B = h->bw;
    *hist = B.S == 1 ? &h->d_hist : &B.hist;
    if (B.S == 1 || B.hist_n >= B.S) return 0;
    if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "run the sequence once before recording it: the first call after dvbs2hip_set_streams allocates the streams' filter memory");
    const size_t nb = sizeof(float) * 2 * (size_t)(h->fir_T > 1 ? h->fir_T - 1 : 1) * (size_t)B.S;
    float *nw[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; i++)
        if (int r = dev_alloc(h, &nw[i], nb, "hipMalloc of the streams' filter memory failed")) { (void)dev_free(h, &nw[0]); return r; }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 2; i++) { (void)dev_free(h, &B.hist.p[i]); B.hist.p[i] = nw[i]; }
    B.hist_n = B.S; B.hist.cur = 0;
    HIPCHK(h, hipMemsetAsync(B.hist.in(), 0, nb, h->stream));
    return 0;
}

extern "C" {

// ------------------------------------------------------------------ a5
// the kernel of a matched-filter call of S streams of n_per samples (fir_choose, rx_dispatch.h); dvbs2hip_set_filter_kernel(h, DVBS2HIP_FIR_VALU) keeps the vector kernel
static FirChoice fir_choice(dvbs2hip_t *h, const float *X, const float *Y, long long n_per, int S)
{
    return fir_choose(h->fir_T, n_per, S, ptr_align(X), ptr_align(Y), h->fir_kernel != DVBS2HIP_FIR_VALU && h->d_fir_afrag);
}

// bw.S streams per call: every stream its own sample stream of n_cplx F/S samples, with its own memory
int dvbs2hip_filter_dev(dvbs2hip_t *h, const float *X, float *Y, int32_t n_cplx, int32_t F)
{
    int r = bw_check(h, F); if (r) return r;
    if (!X || !Y) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if (h->fir_T <= 0) return fail(h, DVBS2HIP_EUNSUPPORTED, "handle was created without filter taps");
    if (n_cplx < 1) return fail(h, DVBS2HIP_EINVAL, "'n_cplx' has to be greater than 0");
    PingPong<float> *hist;
    if ((r = bw_hist(h, &hist))) return r;
    Timer tm(h, DVBS2HIP_K_FIR);
    const long long n_per = (long long)n_cplx * (F / h->bw.S);
    HIPCHK(h, fir_launch(X, Y, hist->in(), hist->out(), h->d_taps_rev, h->d_fir_afrag, h->fir_T, n_per, h->bw.S, fir_choice(h, X, Y, n_per, h->bw.S), h->stream));
    hist->flip();
    return 0;
}

int dvbs2hip_filter(dvbs2hip_t *h, const float *X, float *Y, int32_t n_cplx, int32_t F)
{
    const size_t n = (size_t)2 * (n_cplx > 0 ? n_cplx : 0);
    const auto dev = [&](const float *a, float *b, int nf) { return dvbs2hip_filter_dev(h, a, b, n_cplx, nf); };
    // one stream: chunks of a pinned socket in order; several: the whole call at once (a chunk would cut across the streams)
    return h && h->bw.S > 1 ? host_wrap<false>(h, X, n, Y, n, F, dev) : host_wrap<true>(h, X, n, Y, n, F, dev);
}

// filter1 / filter2: the reference splits the matched filter over two pipeline stages (Filter_FIR_ccr.cpp:144-294; bound
// RX/main_sched.cpp:199-201): filter1 produces the lower part of every frame and advances the state, filter2 copies Y_N2h and
// produces the upper part from X_N1 alone.  Both are pure functions of their sockets here too (they may sit in different
// pipeline stages, working on different batches at the same time).
int dvbs2hip_filter_split(const dvbs2hip_t *h, int32_t n_cplx)
{
    if (!h || h->fir_T <= 0) return DVBS2HIP_EINVAL;
    const int split = (n_cplx / 2) & ~3;                  // 32-byte aligned rows for the 2-D copies
    return split >= h->fir_T - 1 && split < n_cplx ? split : DVBS2HIP_EINVAL;
}

int dvbs2hip_filter1_dev(dvbs2hip_t *h, const float *X, float *Y, int32_t n_cplx, int32_t F)
{
    if (h && dvbs2hip_filter_split(h, n_cplx) < 0) return fail(h, DVBS2HIP_EINVAL, "filter1 / filter2: half a frame has to hold the filter's memory (n_cplx / 2 >= n_taps - 1)");
    // the lower part is all the reference defines for this socket; the upper part of Y_N2, which the reference leaves as it
    // was, is filled too (one stream pass computes both, and filter2 overwrites it anyway)
    return dvbs2hip_filter_dev(h, X, Y, n_cplx, F);
}

int dvbs2hip_filter2_dev(dvbs2hip_t *h, const float *X, const float *Yh, float *Y, int32_t n_cplx, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X || !Yh || !Y) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if (h->fir_T <= 0) return fail(h, DVBS2HIP_EUNSUPPORTED, "handle was created without filter taps");
    const int split = dvbs2hip_filter_split(h, n_cplx);
    if (split < 0) return fail(h, DVBS2HIP_EINVAL, "filter1 / filter2: half a frame has to hold the filter's memory (n_cplx / 2 >= n_taps - 1)");
    const size_t hb = sizeof(float) * 2 * (size_t)(h->fir_T > 1 ? h->fir_T - 1 : 1);
    if (!h->d_hist_zero || !h->d_hist_junk) {      // both buffers, zeroed, or neither: the handle only ever sees the complete pair
        float *z = nullptr, *j = nullptr;
        hipError_t e = dev_malloc(h, &z, hb);
        if (e == hipSuccess) e = dev_malloc(h, &j, hb);
        if (e == hipSuccess) e = hipMemsetAsync(z, 0, hb, h->stream);
        if (e != hipSuccess) { (void)dev_free(h, &z); (void)dev_free(h, &j); HIPCHK(h, e); }
        (void)dev_free(h, &h->d_hist_zero); (void)dev_free(h, &h->d_hist_junk);
        h->d_hist_zero = z; h->d_hist_junk = j;
    }
    void *tmp;
    const size_t row = sizeof(float) * 2 * (size_t)n_cplx;
    if ((r = ensure(h, B_FLT2, row * F, &tmp))) return r;
    {   // the upper part of a frame reads nothing before the frame (split >= n_taps - 1): the state is neither used nor advanced
        Timer tm(h, DVBS2HIP_K_FIR);
        HIPCHK(h, fir_launch(X, (float *)tmp, h->d_hist_zero, h->d_hist_junk, h->d_taps_rev, h->d_fir_afrag, h->fir_T, (long long)n_cplx * F, 1,
                             fir_choice(h, X, (const float *)tmp, (long long)n_cplx * F, 1), h->stream));
    }
    const size_t lo = sizeof(float) * 2 * (size_t)split;
    if (Y != Yh) HIPCHK(h, hipMemcpy2DAsync(Y, row, Yh, row, lo, (size_t)F, hipMemcpyDeviceToDevice, h->stream));       // std::copy(Y_N2h, ..) :224
    HIPCHK(h, hipMemcpy2DAsync((char *)Y + lo, row, (const char *)tmp + lo, row, row - lo, (size_t)F, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

int dvbs2hip_filter1(dvbs2hip_t *h, const float *X, float *Y, int32_t n_cplx, int32_t F)
{
    if (h && dvbs2hip_filter_split(h, n_cplx) < 0) return fail(h, DVBS2HIP_EINVAL, "filter1 / filter2: half a frame has to hold the filter's memory (n_cplx / 2 >= n_taps - 1)");
    return dvbs2hip_filter(h, X, Y, n_cplx, F);
}

int dvbs2hip_filter2(dvbs2hip_t *h, const float *X, const float *Yh, float *Y, int32_t n_cplx, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X || !Yh || !Y) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    const int split = dvbs2hip_filter_split(h, n_cplx);
    if (split < 0) return fail(h, DVBS2HIP_EINVAL, "filter1 / filter2: half a frame has to hold the filter's memory (n_cplx / 2 >= n_taps - 1)");
    const size_t row = sizeof(float) * 2 * (size_t)n_cplx, lo = sizeof(float) * 2 * (size_t)split;
    void *din, *dout;
    if ((r = ensure(h, B_IN, row * F, &din)) || (r = ensure(h, B_OUT, row * F, &dout))) return r;
    HIPCHK(h, hipMemcpyAsync(din, X, row * F, hipMemcpyHostToDevice, h->stream));
    if ((r = dvbs2hip_filter2_dev(h, (const float *)din, (const float *)dout, (float *)dout, n_cplx, F))) return r;     // Yh == Y on the device: lower part untouched
    if (Y != Yh) for (int f = 0; f < F; f++) memcpy((char *)Y + (size_t)f * row, (const char *)Yh + (size_t)f * row, lo);   // std::copy(Y_N2h, ..) :224, lower part
    HIPCHK(h, hipMemcpy2DAsync((char *)Y + lo, row, (const char *)dout + lo, row, row - lo, (size_t)F, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int dvbs2hip_filter_reset(dvbs2hip_t *h)
{
    int r0 = enter(h); if (r0) return r0;
    if (h->fir_T > 1 && h->d_hist_all) {      // buffers 0 become the current ones, zeroed by one memset (they are adjacent); buffers 1 are written before they are read
        HIPCHK(h, hipMemsetAsync(h->d_hist_all, 0, 2 * h->hist_stride, h->stream));
        h->d_hist.cur = 0; h->d_uphist.cur = 0;
    }
    if (h->bw.hist.p[0]) {                     // every stream's memory (dvbs2hip_set_streams)
        h->bw.hist.cur = 0;
        HIPCHK(h, hipMemsetAsync(h->bw.hist.in(), 0, sizeof(float) * 2 * (size_t)(h->fir_T > 1 ? h->fir_T - 1 : 1) * (size_t)h->bw.hist_n, h->stream));
    }
    return 0;
}

// ------------------------------------------------------------------ N2: shaping filter, channel noise, perfect timing
int dvbs2hip_shape_filter_dev(dvbs2hip_t *h, const float *X, float *Y, int32_t n_cplx, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X || !Y) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if (h->fir_T <= 0) return fail(h, DVBS2HIP_EUNSUPPORTED, "handle was created without filter taps");
    if (n_cplx < 1) return fail(h, DVBS2HIP_EINVAL, "'n_cplx' has to be greater than 0");
    Timer tm(h, DVBS2HIP_K_FIR);
    const FirChoice ch = upfir_choose(h->fir_T, h->fir_osf, (long long)n_cplx * F, ptr_align(X), ptr_align(Y), h->fir_kernel != DVBS2HIP_FIR_VALU && h->d_upfir_afrag);
    HIPCHK(h, upfir_launch(X, Y, h->d_uphist.in(), h->d_uphist.out(), h->d_taps, h->d_upfir_afrag, h->fir_T, h->fir_osf, (long long)n_cplx * F, ch, h->stream));
    h->d_uphist.flip();
    return 0;
}

int dvbs2hip_shape_filter(dvbs2hip_t *h, const float *X, float *Y, int32_t n_cplx, int32_t F)
{
    const size_t n = (size_t)2 * (n_cplx > 0 ? n_cplx : 0);
    return host_wrap(h, X, n, Y, n * (h ? h->fir_osf : 1), F, [&](const float *a, float *b, int nf) { return dvbs2hip_shape_filter_dev(h, a, b, n_cplx, nf); });
}

int dvbs2hip_add_noise_dev(dvbs2hip_t *h, const float *CP, const float *X, float *Y, uint64_t seed, int32_t n_elmts, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!CP || !X || !Y) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if (n_elmts < 2 || (n_elmts & 1)) return fail(h, DVBS2HIP_EINVAL, "'n_elmts' has to be a positive even number");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, awgn_launch(X, Y, CP, seed, n_elmts / 2, F, h->stream));
    return 0;
}

int dvbs2hip_add_noise(dvbs2hip_t *h, const float *CP, const float *X, float *Y, uint64_t seed, int32_t n_elmts, int32_t F)
{
    const size_t n4 = (size_t)F * (n_elmts > 0 ? (size_t)n_elmts : 0) * 4;
    return host_call(h, F, false, {{CP, B_SIG, (size_t)F * 4}, {X, B_IN, n4}}, {{Y, B_OUT, n4}},
                     [&](void *const *i, void *const *o, int nf) { return dvbs2hip_add_noise_dev(h, (const float *)i[0], (const float *)i[1], (float *)o[0], seed, n_elmts, nf); });
}

int dvbs2hip_extract_dev(dvbs2hip_t *h, const float *X, float *Y, int32_t n_cplx_out, int32_t osf, int64_t offset, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X || !Y) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if (n_cplx_out < 1 || osf < 1) return fail(h, DVBS2HIP_EINVAL, "'n_cplx_out' and 'osf' have to be greater than 0");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, decimate_launch(X, Y, (long long)n_cplx_out * F, osf, offset, (long long)n_cplx_out * F * osf, h->stream));
    return 0;
}

// ------------------------------------------------------------------ Multiplier_AGC_cc_naive::imultiply (the two gain stages of the reference's RX graph)
int dvbs2hip_agc_imultiply_dev(dvbs2hip_t *h, const float *X, float *Z, int32_t n_cplx, float output_energy, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X || !Z) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if (n_cplx < 1) return fail(h, DVBS2HIP_EINVAL, "'n_cplx' has to be greater than 0");
    if (!(output_energy > 0.f)) return fail(h, DVBS2HIP_EINVAL, "'output_energy' has to be greater than 0");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, agc_launch(X, Z, n_cplx, output_energy, F, h->stream));
    return 0;
}
int dvbs2hip_agc_imultiply(dvbs2hip_t *h, const float *X, float *Z, int32_t n_cplx, float output_energy, int32_t F)
{
    const size_t n = (size_t)2 * (n_cplx > 0 ? n_cplx : 0);
    return host_wrap<true>(h, X, n, Z, n, F, [&](const float *a, float *b, int nf) { return dvbs2hip_agc_imultiply_dev(h, a, b, n_cplx, output_energy, nf); });
}

}  // extern "C"
