// The C ABI of the transmitter's tasks (include/dvbs2hip.h, "TX tasks"): one entry per codelet the reference's TX mains bind between the source and
// the shaping filter, a host form and a _dev form each, as the RX twins in dvbs2hip_api.hip.  Kernels: k_tx_tasks.hip (and, for the BB scrambler, the
// launch its inverse uses).  The tasks keep no state; the BCH encoder's packed message lives in the handle's B_TXBCH scratch for the length of the call.
#include "dvbs2hip_handle.h"

using namespace dvbs2;

// what the two encoders read of the handle (the fused dvbs2hip_tx_bb fills the same structure, with its sockets)
static int tx_task_params(dvbs2hip_t *h, int F, bool bch_scratch, TxKParams &p)
{
    memset(&p, 0, sizeof p);
    if (bch_scratch) {
        void *dbch;
        if (int r = ensure(h, B_TXBCH, (size_t)F * ((h->K_ldpc + 31) / 32) * 4, &dbch)) return r;
        p.bch_cw = (uint32_t *)dbch;
    }
    p.enc_tab = h->d_enc_tab; p.enc_deg = h->d_enc_deg; p.bch_tab = h->d_bch_tab; p.bch_shift = h->d_bch_shift;
    p.K_bch = h->K_bch; p.K_ldpc = h->K_ldpc; p.N_ldpc = h->N_ldpc; p.bps = h->bps; p.itl_cols = h->itl_cols; p.itl_order = h->itl_order;
    p.n_sym = h->n_sym; p.pl_frame = h->pl_frame; p.enc_stride = h->enc_stride; p.n_frames = F;
    return 0;
}

extern "C" {

// ------------------------------------------------------------------ Scrambler_BB::scramble
int dvbs2hip_bb_scramble_dev(dvbs2hip_t *h, const int32_t *a, int32_t *b, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!a || !b) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, bb_descramble_launch(a, b, h->bch.d_prbs, h->K_bch, F, h->stream));      // the same XOR both ways
    return 0;
}
int dvbs2hip_bb_scramble(dvbs2hip_t *h, const int32_t *a, int32_t *b, int32_t F)
{
    const size_t n = h ? (size_t)h->K_bch : 0;
    return host_wrap<true>(h, a, n, b, n, F, [&](const int32_t *x, int32_t *y, int nf) { return dvbs2hip_bb_scramble_dev(h, x, y, nf); });
}

// ------------------------------------------------------------------ Encoder_BCH_DVBS2::encode
int dvbs2hip_bch_encode_dev(dvbs2hip_t *h, const int32_t *U, int32_t *X, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!U || !X) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    TxKParams p;
    if ((r = tx_task_params(h, F, true, p))) return r;
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, tx_bch_encode_launch(p, U, X, h->stream));
    return 0;
}
int dvbs2hip_bch_encode(dvbs2hip_t *h, const int32_t *U, int32_t *X, int32_t F)
{
    // (the chunks of a pinned call share the packed scratch: they follow one another on the handle's stream)
    return host_wrap<true>(h, U, h ? (size_t)h->K_bch : 0, X, h ? (size_t)h->K_ldpc : 0, F,
                           [&](const int32_t *x, int32_t *y, int nf) { return dvbs2hip_bch_encode_dev(h, x, y, nf); });
}

// ------------------------------------------------------------------ the LDPC encoder
int dvbs2hip_ldpc_encode_dev(dvbs2hip_t *h, const int32_t *U, int32_t *X, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!U || !X) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    TxKParams p;
    if ((r = tx_task_params(h, F, false, p))) return r;
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, tx_ldpc_encode_launch(p, U, X, h->stream));
    return 0;
}
int dvbs2hip_ldpc_encode(dvbs2hip_t *h, const int32_t *U, int32_t *X, int32_t F)
{
    return host_wrap<true>(h, U, h ? (size_t)h->K_ldpc : 0, X, h ? (size_t)h->N_ldpc : 0, F,
                           [&](const int32_t *x, int32_t *y, int nf) { return dvbs2hip_ldpc_encode_dev(h, x, y, nf); });
}

// ------------------------------------------------------------------ Interleaver::interleave
int dvbs2hip_interleave_dev(dvbs2hip_t *h, const int32_t *nat, int32_t *itl, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!nat || !itl) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, tx_interleave_launch(nat, itl, h->N_ldpc, h->itl_cols, h->itl_order, F, h->stream));
    return 0;
}
int dvbs2hip_interleave(dvbs2hip_t *h, const int32_t *nat, int32_t *itl, int32_t F)
{
    const size_t n = h ? (size_t)h->N_ldpc : 0;
    return host_wrap<true>(h, nat, n, itl, n, F, [&](const int32_t *x, int32_t *y, int nf) { return dvbs2hip_interleave_dev(h, x, y, nf); });
}

// ------------------------------------------------------------------ Modem::modulate
int dvbs2hip_modulate_dev(dvbs2hip_t *h, const int32_t *X1, float *X2, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X1 || !X2) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, tx_modulate_launch(X1, X2, h->d_cstl, h->bps, h->N_ldpc, h->n_sym, F, h->stream));
    return 0;
}
int dvbs2hip_modulate(dvbs2hip_t *h, const int32_t *X1, float *X2, int32_t F)
{
    return host_wrap<true>(h, X1, h ? (size_t)h->N_ldpc : 0, X2, h ? (size_t)2 * h->n_sym : 0, F,
                           [&](const int32_t *x, float *y, int nf) { return dvbs2hip_modulate_dev(h, x, y, nf); });
}

// ------------------------------------------------------------------ Framer::generate
int dvbs2hip_framer_generate_dev(dvbs2hip_t *h, const float *Y1, float *Y2, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!Y1 || !Y2) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, tx_framer_launch(Y1, Y2, h->d_plh, h->n_sym, h->pl_frame, F, h->stream));
    return 0;
}
int dvbs2hip_framer_generate(dvbs2hip_t *h, const float *Y1, float *Y2, int32_t F)
{
    return host_wrap<true>(h, Y1, h ? (size_t)2 * h->n_sym : 0, Y2, h ? (size_t)2 * h->pl_frame : 0, F,
                           [&](const float *x, float *y, int nf) { return dvbs2hip_framer_generate_dev(h, x, y, nf); });
}

// ------------------------------------------------------------------ Scrambler_PL::scramble
int dvbs2hip_pl_scramble_dev(dvbs2hip_t *h, const float *X1, float *X2, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X1 || !X2) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, tx_pl_scramble_launch(X1, X2, h->d_pl_seq, h->pl_frame, F, h->stream));
    return 0;
}
int dvbs2hip_pl_scramble(dvbs2hip_t *h, const float *X1, float *X2, int32_t F)
{
    const size_t n = h ? (size_t)2 * h->pl_frame : 0;
    return host_wrap<true>(h, X1, n, X2, n, F, [&](const float *x, float *y, int nf) { return dvbs2hip_pl_scramble_dev(h, x, y, nf); });
}

}  // extern "C"
