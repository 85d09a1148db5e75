// C ABI, the receiver's frame-level synchronizers: frame synchronizer (sfm_*), L&R fine frequency and pilot phase (sff_call, lr_*).
#include "dvbs2hip_handle.h"

using namespace dvbs2;

// L&R timeout (sff_lr_fused_kernel): every estimate has been published by the time the launch is over, so the rotation alone is run again (the stores
// the waiting workgroups dropped) -- with the estimates of THAT launch (the slot's own buffer).  The caller has synchronized the stream.  Returns 0 when there was
// nothing to do or the recovery succeeded.
static int lr_check_recover(dvbs2hip_t *h, int slot)
{
    auto &ls = h->lr_slot[slot];
    ls.pending = false;
    if (!h->lr_err_host || !((volatile uint32_t *)h->lr_err_host)[slot]) return 0;
    ((volatile uint32_t *)h->lr_err_host)[slot] = 0u;
    h->lr_timeouts++;
    auto it = h->bufs.find(B_LR_TMP0 + slot);
    if (!ls.x || !ls.y || it == h->bufs.end() || !it->second.p || it->second.bytes < sizeof(float) * 4 * (size_t)ls.F)
        return fail(h, DVBS2HIP_EHIP, "L&R: a rotating workgroup timed out waiting for the recurrence and the call cannot be repeated (buffers unknown); re-run it with DVBS2HIP_LR=unfused");
    HIPCHK(h, sff_lr_recover(ls.x, ls.y, (float *)it->second.p, ls.n, ls.F, rotate_choose(ls.n, ptr_align(ls.x), ptr_align(ls.y)), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// every device-form L&R call that has not been looked at yet, oldest first (the stream is synchronized here)
int dvbs2::lr_check_all(dvbs2hip_t *h)
{
    bool any = false;
    for (int i = 0; i < dvbs2hip_handle::LR_SLOTS; i++) any |= h->lr_slot[i].pending;
    if (!any) return 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int r = 0;
    for (int i = 0; i < dvbs2hip_handle::LR_SLOTS; i++) {
        const int s = (h->lr_next + i) % dvbs2hip_handle::LR_SLOTS;          // lr_next is the oldest slot
        if (h->lr_slot[s].pending) { const int ri = lr_check_recover(h, s); if (ri && !r) r = ri; }
    }
    return r;
}

extern "C" {

// ------------------------------------------------------------------ N4: frame synchronizer (Synchronizer_frame_DVBS2_fast)
// the kernels of a call of Fs frames per stream (sync_choose, rx_dispatch.h, which reads DVBS2HIP_SYNC* at every call)
static SyncChoice sfm_choice(dvbs2hip_t *h, const float *X_N1, int Fs, bool one_task, bool located)
{
    return sync_choose({h->pl_frame, Fs, h->bw.S, h->sfm.nbuff2, ptr_align(X_N1), h->sfm.frag != nullptr, h->sfm.keys != nullptr, one_task, located});
}

// every stream the state holds (S.n_alloc of them, side by side: dvbs2hip_set_streams)
static int sfm_state_reset(dvbs2hip_t *h, bool all)
{
    const int n = h->pl_frame;
    auto &S = h->sfm;
    const size_t ns = (size_t)S.n_alloc;
    std::vector<float> xh0(ns * 2 * 64, 0.f);
    std::vector<int> st0(ns * SYNC_ST_STRIDE, 0);
    for (size_t s = 0; s < ns; s++) {
        xh0[s * 128 + 2 * 63] = 1.f;                                               // reg_channel = (1, 0), .cpp:19 / :309
        st0[s * SYNC_ST_STRIDE + 1] = 1;                                           // head2 = 0, first_time = true
    }
    for (int i = 0; i < 2; i++) {
        HIPCHK(h, hipMemsetAsync(S.xh.p[i], 0, sizeof(float) * 2 * 64 * ns, h->stream));
        HIPCHK(h, hipMemsetAsync(S.buff2.p[i], 0, sizeof(float) * (size_t)S.nbuff2 * ns, h->stream));
        HIPCHK(h, hipMemcpyAsync(S.st.p[i], st0.data(), sizeof(int) * st0.size(), hipMemcpyHostToDevice, h->stream));
        if (all) HIPCHK(h, hipMemsetAsync(S.sofh.p[i], 0, sizeof(float) * 2 * 64 * ns, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(S.xh.in(), xh0.data(), sizeof(float) * xh0.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(S.cv, 0, sizeof(float) * (size_t)n * ns, h->stream));
    if (all) { HIPCHK(h, hipMemsetAsync(S.yprev.in(), 0, sizeof(float) * 2 * (size_t)n * ns, h->stream)); HIPCHK(h, hipMemsetAsync(S.metric, 0, sizeof(float) * ns, h->stream)); }
    HIPCHK(h, hipStreamSynchronize(h->stream));                                    // `xh0` / `st0` live on this stack
    return 0;
}

// the per-stream state for ns streams, side by side: a complete set or nothing (a failure leaves the handle with what it had)
static int sfm_alloc_streams(dvbs2hip_t *h, int ns)
{
    auto &S = h->sfm;
    const int n = h->pl_frame;
    const size_t z = (size_t)ns;
    float *xh[2] = {}, *sofh[2] = {}, *buff2[2] = {}, *yprev[2] = {}, *cv = nullptr, *metric = nullptr;
    int *st[2] = {};
    const char *what = "hipMalloc of the frame synchronizer's per-stream state failed";
    int r = 0;
    for (int i = 0; i < 2 && !r; i++)
        if ((r = dev_alloc(h, &xh[i], sizeof(float) * 2 * 64 * z, what)) || (r = dev_alloc(h, &sofh[i], sizeof(float) * 2 * 64 * z, what)) ||
            (r = dev_alloc(h, &buff2[i], sizeof(float) * (size_t)S.nbuff2 * z, what)) || (r = dev_alloc(h, &st[i], sizeof(int) * SYNC_ST_STRIDE * z, what)) ||
            (r = dev_alloc(h, &yprev[i], sizeof(float) * 2 * (size_t)n * z, what))) break;
    if (!r && !(r = dev_alloc(h, &cv, sizeof(float) * (size_t)n * z, what))) r = dev_alloc(h, &metric, sizeof(float) * z, what);
    if (r) {
        for (int i = 0; i < 2; i++) { (void)dev_free(h, &xh[i]); (void)dev_free(h, &sofh[i]); (void)dev_free(h, &buff2[i]); (void)dev_free(h, &st[i]); (void)dev_free(h, &yprev[i]); }
        (void)dev_free(h, &cv); (void)dev_free(h, &metric);
        return r;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 2; i++) {
        (void)dev_free(h, &S.xh.p[i]); (void)dev_free(h, &S.sofh.p[i]); (void)dev_free(h, &S.buff2.p[i]); (void)dev_free(h, &S.st.p[i]); (void)dev_free(h, &S.yprev.p[i]);
        S.xh.p[i] = xh[i]; S.sofh.p[i] = sofh[i]; S.buff2.p[i] = buff2[i]; S.st.p[i] = st[i]; S.yprev.p[i] = yprev[i];
    }
    (void)dev_free(h, &S.cv); (void)dev_free(h, &S.metric);
    S.cv = cv; S.metric = metric;
    S.n_alloc = ns;
    S.xh.cur = S.sofh.cur = S.buff2.cur = S.st.cur = S.yprev.cur = 0;
    return sfm_state_reset(h, true);
}

static int sfm_ready(dvbs2hip_t *h)
{
    auto &S = h->sfm;
    if (S.ready && S.n_alloc >= h->bw.S) return 0;
    if (h->capturing && S.ready) return fail(h, DVBS2HIP_EINVAL, "run the sequence once before recording it: the first call after dvbs2hip_set_streams allocates the streams' state");
    const int n = h->pl_frame;
    S.nbuff2 = 4 * (n + 1);                                                        // Variable_delay_cc_naive(N, N/2, N/2): buff2(4 (max_delay + 1))
    if (!S.keys)
        DEV_ALLOC_CHK(h, &S.keys, sizeof(unsigned long long) * (size_t)h->max_frames * (size_t)((n + 63) / 64) + sizeof(float) * 2 * (size_t)((h->max_frames + SYNC_SUB - 1) / SYNC_SUB) * (size_t)n);      // (+ the segments' {A, B} of the average over frames: k_sync.hip)
    if (!S.frag) {
        const std::vector<uint16_t> fr = sync_frag_default();
        DEV_ALLOC_CHK(h, &S.frag, fr.size() * sizeof(uint16_t));
        HIPCHK(h, hipMemcpy(S.frag, fr.data(), fr.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    int r = sfm_alloc_streams(h, h->bw.S);                                        // (it leaves every stream in the reset state)
    if (r) return r;
    S.ready = true;
    return 0;
}

int dvbs2hip_sync_frame_set_params(dvbs2hip_t *h, float alpha, float trigger, int32_t vec_width)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (vec_width < 1) return fail(h, DVBS2HIP_EINVAL, "'vec_width' has to be greater than 0");
    h->sfm.alpha = alpha; h->sfm.trigger = trigger; h->sfm.vec_width = vec_width;
    return 0;
}

int dvbs2hip_sync_frame_reset(dvbs2hip_t *h)
{
    int r;
    if ((r = enter(h)) || (r = sfm_ready(h))) return r;
    return sfm_state_reset(h, false);                                              // .cpp:304-318: SOF_PLSC_delay keeps its memory
}

int dvbs2hip_sync_frame_synchronize1_dev(dvbs2hip_t *h, const float *X_N1, float *cor_SOF, float *cor_PLSC, int32_t F)
{
    int r = bw_check(h, F); if (r) return r;
    if (!X_N1 || !cor_SOF || !cor_PLSC) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if ((r = sfm_ready(h))) return r;
    auto &S = h->sfm;
    Timer tm(h, DVBS2HIP_K_MISC);
    // every stream from its own 64-sample memory
    const int Fs = F / h->bw.S;
    HIPCHK(h, sync_corr_launch(X_N1, S.xh.in(), S.xh.out(), S.frag, cor_SOF, cor_PLSC, (long long)h->pl_frame * Fs, h->bw.S, sfm_choice(h, X_N1, Fs, false, false), h->stream));
    S.xh.flip();
    return 0;
}

// synchronize2, or (cor_SOF == cor_PLSC == null) the whole one-task synchronize with the correlators fused into the metric
static int sfm_sync2(dvbs2hip_t *h, const float *X_N1, const float *cor_SOF, const float *cor_PLSC, int32_t *DEL, int32_t *FLG, float *TRI, float *Y_N2, int32_t F, const float **SRC = nullptr)
{
    int r = bw_check(h, F); if (r) return r;
    const int NS = h->bw.S, Fs = F / NS;                                           // streams of the call, frames per stream
    if (SRC && NS > 1) return fail(h, DVBS2HIP_EUNSUPPORTED, "the located form of the frame synchronizer is one stream per handle: with dvbs2hip_set_streams(S > 1) use dvbs2hip_sync_frame_synchronize_dev");
    int32_t *delay = DEL;
    const bool fused = !cor_SOF && !cor_PLSC;
    if (!X_N1 || (!fused && (!cor_SOF || !cor_PLSC)) || !delay || (!Y_N2 && !SRC)) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if ((r = sfm_ready(h))) return r;
    auto &S = h->sfm;
    const int n = h->pl_frame;
    const SyncChoice ch = sfm_choice(h, X_N1, Fs, fused, SRC != nullptr);
    if (fused && !ch.fused) {      // the two tasks through device scratch (same numbers)
        const size_t nb = sizeof(float) * 2 * (size_t)n * F;
        void *cs, *cp;
        if ((r = ensure(h, B_SFM_SOF, nb, &cs)) || (r = ensure(h, B_SFM_PLSC, nb, &cp))) return r;
        if ((r = dvbs2hip_sync_frame_synchronize1_dev(h, X_N1, (float *)cs, (float *)cp, F))) return r;
        return dvbs2hip_sync_frame_synchronize2_dev(h, X_N1, (const float *)cs, (const float *)cp, DEL, FLG, TRI, Y_N2, F);
    }
    void *corr, *met;
    void *dtab;
    if ((r = ensure(h, B_SFM_CORR, sizeof(float) * (size_t)n * F, &corr)) || (r = ensure(h, B_SFM_MET, sizeof(float) * (size_t)F, &met)) ||
        (r = ensure(h, B_SFM_DTAB, sizeof(int32_t) * (size_t)F, &dtab))) return r;
    Timer tm(h, DVBS2HIP_K_MISC);
    if (TRI) met = TRI;
    const SyncTail tail{S.keys, delay, (float *)met, FLG, S.trigger, (int32_t *)dtab, S.metric, reinterpret_cast<float *>(S.keys + (size_t)h->max_frames * (size_t)((n + 63) / 64))};
    // every stream on its own state; frame 0 of a stream continues from that stream's previous call
    if (fused) {
        HIPCHK(h, sync_corr_metric_launch(X_N1, S.xh.in(), S.xh.out(), S.frag, S.sofh.in(), S.sofh.out(), S.cv, (float *)corr, tail, n, Fs, NS, S.alpha, S.vec_width, ch, h->stream));
        S.xh.flip();
    } else
        HIPCHK(h, sync_metric_launch(cor_SOF, S.sofh.in(), S.sofh.out(), cor_PLSC, S.cv, (float *)corr, tail, n, Fs, NS, S.alpha, S.vec_width, ch, h->stream));
    S.sofh.flip();
    // the delay line is a recurrence from frame to frame made of copies only: resolved per output sample, one launch (k_sync.hip)
    void *need = nullptr;
    if (SRC) {      // located form: only the frames that are not a run of the input stream are materialized (into the handle's scratch); SRC[f] says where frame f starts
        void *scr;
        if ((r = ensure(h, B_SFM_SCR, sizeof(float) * 2 * (size_t)n * F, &scr)) || (r = ensure(h, B_SFM_NEED, sizeof(int32_t) * ((size_t)F + 2), &need))) return r;
        Y_N2 = (float *)scr;
    }
    HIPCHK(h, sync_vdelay_launch(X_N1, S.yprev.in(), S.yprev.out(), Y_N2, S.buff2.in(), S.buff2.out(), S.st.in(), S.st.out(), (const int32_t *)dtab, n, S.nbuff2, Fs, NS, ch,
                                 h->stream, (int32_t *)need, SRC));
    S.buff2.flip(), S.st.flip();
    S.yprev.flip();
    return 0;
}

int dvbs2hip_sync_frame_synchronize2_dev(dvbs2hip_t *h, const float *X_N1, const float *cor_SOF, const float *cor_PLSC, int32_t *DEL, int32_t *FLG,
                                         float *TRI, float *Y_N2, int32_t F)
{
    if (h && (!cor_SOF || !cor_PLSC)) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    return sfm_sync2(h, X_N1, cor_SOF, cor_PLSC, DEL, FLG, TRI, Y_N2, F);
}

int dvbs2hip_sync_frame_synchronize_dev(dvbs2hip_t *h, const float *X_N1, int32_t *DEL, int32_t *FLG, float *TRI, float *Y_N2, int32_t F)
{
    // the one-task form: the two correlations are no sockets here and stay on chip (sync_corr_m_kernel), unless sync_choose says otherwise
    return sfm_sync2(h, X_N1, nullptr, nullptr, DEL, FLG, TRI, Y_N2, F);
}

// (round 5) the frame synchronizer for a consumer of this library: instead of the delayed copy Y_N2 it returns, per frame, WHERE the aligned frame starts -- inside X_N1 for a
// frame that is one run of the input stream (every frame in lock but the first and the last of a call), inside the handle's scratch for the others.  X_N1 and the table stay
// valid until the next synchronizer call on this handle; the frames are 8-byte aligned.  DEL / FLG / TRI and the synchronizer's state are those of `synchronize`.
int dvbs2hip_sync_frame_locate_dev(dvbs2hip_t *h, const float *X_N1, int32_t *DEL, int32_t *FLG, float *TRI, const float **SRC, int32_t F)
{
    if (h && !SRC) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if (h && h->bw.S > 1) return fail(h, DVBS2HIP_EUNSUPPORTED, "the located form of the frame synchronizer is one stream per handle: with dvbs2hip_set_streams(S > 1) use dvbs2hip_sync_frame_synchronize_dev");
    return sfm_sync2(h, X_N1, nullptr, nullptr, DEL, FLG, TRI, nullptr, F, SRC);
}

int dvbs2hip_sync_frame_synchronize1(dvbs2hip_t *h, const float *X_N1, float *cor_SOF, float *cor_PLSC, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    const size_t nb = sizeof(float) * 2 * (size_t)h->pl_frame * F;
    return host_call(h, F, false, {{X_N1, B_IN, nb}}, {{cor_SOF, B_SFM_SOF, nb}, {cor_PLSC, B_SFM_PLSC, nb}},
                     [&](void *const *i, void *const *o, int nf) { return dvbs2hip_sync_frame_synchronize1_dev(h, (const float *)i[0], (float *)o[0], (float *)o[1], nf); });
}

// host-socket forms of synchronize2 / synchronize: DEL, FLG, TRI have one entry per frame (Synchronizer_frame.hxx:42-44); FLG, TRI may be NULL
static int sfm_host(dvbs2hip_t *h, const float *X_N1, const float *cor_SOF, const float *cor_PLSC, int32_t *DEL, int32_t *FLG, float *TRI, float *Y_N2, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    const size_t nb = sizeof(float) * 2 * (size_t)h->pl_frame * F, nf4 = 4 * (size_t)F;
    return host_call(h, F, false, {{X_N1, B_IN, nb}, {cor_SOF, B_SFM_SOF, nb, 0, true}, {cor_PLSC, B_SFM_PLSC, nb, 0, true}},
                     {{DEL, B_SFM_DLY, nf4}, {FLG, B_SFM_DLY, nf4, nf4, true}, {TRI, B_SFM_DLY, nf4, 2 * nf4, true}, {Y_N2, B_OUT, nb}}, [&](void *const *i, void *const *o, int nf) {
        if (cor_SOF) return dvbs2hip_sync_frame_synchronize2_dev(h, (const float *)i[0], (const float *)i[1], (const float *)i[2], (int32_t *)o[0], (int32_t *)o[1], (float *)o[2], (float *)o[3], nf);
        return dvbs2hip_sync_frame_synchronize_dev(h, (const float *)i[0], (int32_t *)o[0], (int32_t *)o[1], (float *)o[2], (float *)o[3], nf);
    });
}

int dvbs2hip_sync_frame_synchronize2(dvbs2hip_t *h, const float *X_N1, const float *cor_SOF, const float *cor_PLSC, int32_t *DEL, int32_t *FLG,
                                     float *TRI, float *Y_N2, int32_t F)
{
    if (h && (!cor_SOF || !cor_PLSC)) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    return sfm_host(h, X_N1, cor_SOF, cor_PLSC, DEL, FLG, TRI, Y_N2, F);
}

int dvbs2hip_sync_frame_synchronize(dvbs2hip_t *h, const float *X_N1, int32_t *DEL, int32_t *FLG, float *TRI, float *Y_N2, int32_t F)
{
    return sfm_host(h, X_N1, nullptr, nullptr, DEL, FLG, TRI, Y_N2, F);
}

// ------------------------------------------------------------------ N4: fine frequency / phase synchronizers (sockets X_N1, FRQ, PHS, Y_N2)
static int sff_call(dvbs2hip_t *h, bool lr, bool host, const float *X_N1, float *FRQ, float *PHS, float *Y_N2, int32_t F)
{
    int r = lr ? bw_check(h, F) : check_frames(h, F); if (r) return r;
    if (!X_N1 || !Y_N2) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    const int n = h->pl_frame;
    if (n <= 1530) return fail(h, DVBS2HIP_EUNSUPPORTED, "the PL frame holds no pilot block");
    const int NS = lr ? h->bw.S : 1;
    if (lr && h->lr_n < NS) {      // the damped autocorrelation of every stream, zero (a larger stream count comes through dvbs2hip_set_streams, which has cleared the old ones)
        if (h->capturing && h->d_lr_R) return fail(h, DVBS2HIP_EINVAL, "run the sequence once before recording it: the first L&R call after dvbs2hip_set_streams allocates the streams' state");
        float *R = nullptr;
        if ((r = dev_alloc(h, &R, 2 * sizeof(float) * (size_t)NS, "hipMalloc of L&R's per-stream state failed"))) return r;
        if (h->d_lr_R) { HIPCHK(h, hipStreamSynchronize(h->stream)); (void)dev_free(h, &h->d_lr_R); }
        h->d_lr_R = R; h->lr_n = NS;
        HIPCHK(h, hipMemsetAsync(h->d_lr_R, 0, 2 * sizeof(float) * (size_t)NS, h->stream));
    }
    if (lr && !h->lr_err_host) {
        HIPCHK(h, hipHostMalloc((void **)&h->lr_err_host, dvbs2hip_handle::LR_SLOTS * sizeof(uint32_t), hipHostMallocMapped));
        for (int i = 0; i < dvbs2hip_handle::LR_SLOTS; i++) h->lr_err_host[i] = 0u;
        HIPCHK(h, hipHostGetDevicePointer((void **)&h->lr_err_dev, h->lr_err_host, 0));
    }
    const size_t nb = sizeof(float) * 2 * (size_t)n * F, nf4 = sizeof(float) * (size_t)F;
    void *tmp;
    // the estimates: the pilot-phase synchronizer's buffer is its own; an L&R call takes the next of LR_SLOTS slots (estimates + error word).  A slot whose last
    // device-form call has not been looked at yet (LR_SLOTS such calls without a dvbs2hip_synchronize between them) is looked at first -- one stream synchronization,
    // and only then -- so that its repair never meets estimates of another launch
    const int slot = lr ? h->lr_next : 0;
    if (lr) {
        if (h->lr_slot[slot].pending) { HIPCHK(h, hipStreamSynchronize(h->stream)); if ((r = lr_check_recover(h, slot))) return r; }
        h->lr_next = (slot + 1) % dvbs2hip_handle::LR_SLOTS;
    }
    if ((r = ensure(h, lr ? B_LR_TMP0 + slot : B_SFF_TMP, sizeof(float) * 4 * (size_t)F, &tmp))) return r;
    auto launch = [&](const float *x, float *frq, float *phs, float *y) {
        Timer tm(h, DVBS2HIP_K_MISC);
        if (lr) HIPCHK(h, sff_lr_launch(x, y, h->d_lr_R, (float *)tmp, frq, phs, n, F, NS, h->lr_alpha, h->lr_err_dev + slot, lr_choose(NS, n, ptr_align(x), ptr_align(y)), h->stream));
        else HIPCHK(h, sff_fp_launch(x, y, (float *)tmp, frq, phs, n, F, rotate_choose(n, ptr_align(x), ptr_align(y)), h->stream));
        if (lr) { auto &ls = h->lr_slot[slot]; ls.x = x; ls.y = y; ls.n = n; ls.F = F; ls.pending = !host && NS == 1; }      // (NS > 1 is three kernels: no waiting workgroup, nothing to look at later)
        return 0;
    };
    if (!host) return launch(X_N1, FRQ, PHS, Y_N2);
    if ((r = lr_check_all(h))) return r;          // (the host form reuses B_IN / B_OUT: nothing of an earlier device-form call is left pending behind it)
    void *dout = nullptr;
    r = host_call(h, F, false, {{X_N1, B_IN, nb}}, {{Y_N2, B_OUT, nb}, {FRQ, B_SFF_OUT, nf4, 0, true}, {PHS, B_SFF_OUT, nf4, nf4, true}},
                  [&](void *const *i, void *const *o, int) { dout = o[0]; return launch((const float *)i[0], (float *)o[1], (float *)o[2], (float *)o[0]); });
    if (r) return r;
    if (lr && h->lr_err_host && ((volatile uint32_t *)h->lr_err_host)[slot]) {      // timeout in the fused L&R launch: rotate again, copy again
        if ((r = lr_check_recover(h, slot))) return r;
        HIPCHK(h, hipMemcpyAsync(Y_N2, dout, nb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return 0;
}

int dvbs2hip_sync_lr_synchronize(dvbs2hip_t *h, const float *X_N1, float *FRQ, float *PHS, float *Y_N2, int32_t F) { return sff_call(h, true, true, X_N1, FRQ, PHS, Y_N2, F); }
int dvbs2hip_sync_lr_synchronize_dev(dvbs2hip_t *h, const float *X_N1, float *FRQ, float *PHS, float *Y_N2, int32_t F) { return sff_call(h, true, false, X_N1, FRQ, PHS, Y_N2, F); }
int dvbs2hip_sync_freq_phase_synchronize(dvbs2hip_t *h, const float *X_N1, float *FRQ, float *PHS, float *Y_N2, int32_t F) { return sff_call(h, false, true, X_N1, FRQ, PHS, Y_N2, F); }
int dvbs2hip_sync_freq_phase_synchronize_dev(dvbs2hip_t *h, const float *X_N1, float *FRQ, float *PHS, float *Y_N2, int32_t F) { return sff_call(h, false, false, X_N1, FRQ, PHS, Y_N2, F); }

int dvbs2hip_sync_lr_set_alpha(dvbs2hip_t *h, float alpha)
{
    if (!h) return DVBS2HIP_EINVAL;
    h->lr_alpha = alpha;
    return 0;
}

int dvbs2hip_sync_lr_timeouts(dvbs2hip_t *h, int32_t *n)
{
    if (!h || !n) return DVBS2HIP_EINVAL;
    *n = h->lr_timeouts;
    return 0;
}

int dvbs2hip_sync_lr_reset(dvbs2hip_t *h)          // Synchronizer_Luise_Reggiannini_DVBS2_aib::_reset, .cpp:170-176
{
    int r = enter(h); if (r) return r;
    if (h->d_lr_R) HIPCHK(h, hipMemsetAsync(h->d_lr_R, 0, 2 * sizeof(float) * (size_t)h->lr_n, h->stream));      // every stream's
    return 0;
}

// S streams per call in every receive task that keeps a memory: the timing tasks' count (stm.S) and the block-wise tasks' (bw.S); every stream of all of them starts over
int dvbs2hip_set_streams(dvbs2hip_t *h, int32_t S)
{
    int r = enter(h); if (r) return r;
    if (S < 1 || S > h->max_frames || S > 65535) return fail(h, DVBS2HIP_EINVAL, "'S' has to be in [1, min(max_frames, 65535)] ('S' = " + std::to_string(S) + ").");
    if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "a capture is open on this handle");
    if ((r = lr_check_all(h))) return r;                                           // (one-launch L&R calls not looked at yet belong to the old count)
    if ((r = dvbs2hip_sync_timing_set_streams(h, S))) return r;
    h->bw.S = S;                                                                   // (the per-stream state of the new count is allocated by the first call that needs it)
    if ((r = dvbs2hip_filter_reset(h)) || (r = dvbs2hip_sync_lr_reset(h)) || (r = dvbs2hip_estimate_pilots_reset(h))) return r;
    if (h->sfm.ready && (r = sfm_state_reset(h, true))) return r;                  // as a new handle: the SOF delay, the previous output frame and the last metric too
    return 0;
}

int dvbs2hip_sync_frame_get_metric(dvbs2hip_t *h, float *max_corr, int32_t *packet_flag)
{
    if (!h || !max_corr || !packet_flag) return DVBS2HIP_EINVAL;
    if (hipSetDevice(h->device) != hipSuccess) return fail(h, DVBS2HIP_EHIP, "hipSetDevice failed");
    int r = sfm_ready(h); if (r) return r;
    std::vector<float> m((size_t)h->bw.S, 0.f);                                    // one entry per stream (dvbs2hip_set_streams)
    HIPCHK(h, hipMemcpyAsync(m.data(), h->sfm.metric, sizeof(float) * m.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t s = 0; s < m.size(); s++) { max_corr[s] = m[s]; packet_flag[s] = m[s] > h->sfm.trigger ? 1 : 0; }      // _get_metric / _get_packet_flag, .hpp:59-60
    return 0;
}

}  // extern "C"
