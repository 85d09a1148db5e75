// C ABI, the BBFRAME layer (k_bbframe.hip): user packets into BBFRAMEs (BBHEADER, CRC-8 slots, padding) in front of the BB scrambler, and BBFRAMEs back into packets
// behind the BB descrambler, with the header's and the packets' CRC-8 checked.  An extension with no reference task.  Both tasks carry state from call to call, in device
// memory of the handle: one allocation made by the first call, two buffers per task (a launch reads one and writes the other), five counters.
#include "dvbs2hip_handle.h"

using namespace dvbs2;

static int bbf_D(const dvbs2hip_t *h) { return (h->K_bch - 80) / 8; }                      // bytes of a full data field
static size_t bbf_rx_bytes(const dvbs2hip_t *h) { return BBF_RX_HEAD + ((size_t)h->K_bch / 8 + 15) / 16 * 16; }      // (a packet is at most a data field)
static BbfParams bbf_params(const dvbs2hip_t *h) { return {h->K_bch, h->bbf.upl_bits / 8, h->bbf.sync, h->bbf.matype1 << 8 | h->bbf.matype2, h->bbf.mark_tei}; }
static int bbf_capacity(const dvbs2hip_t *h, int F)
{
    // packets lie side by side in the call's F D bytes and the pending packet's at most UPLB, and the last one emitted has its CRC slot behind it
    const long long uplb = h->bbf.upl_bits / 8;
    return (int)(((long long)F * bbf_D(h) + uplb - 1) / uplb);
}

// [tx 0 | tx 1 | rx 0 | rx 1 | counters], zero = reset
static int bbf_state(dvbs2hip_t *h)
{
    if (h->bbf.all) return 0;
    if (h->K_bch % 8 || h->K_bch < 96) return fail(h, DVBS2HIP_EUNSUPPORTED, "the BBFRAME layer needs K_bch to be a whole number of bytes behind the 80-bit header");
    if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "run the sequence once before recording it: the first bbframe call allocates the tasks' state");
    const size_t rxb = bbf_rx_bytes(h), bytes = 2 * BBF_TX_STATE + 2 * rxb + 5 * sizeof(unsigned long long);
    char *p = nullptr;
    if (int r = dev_alloc(h, &p, bytes, "hipMalloc of the BBFRAME tasks' state failed")) return r;
    hipError_t e = hipMemsetAsync(p, 0, bytes, h->stream);
    if (e != hipSuccess) { (void)dev_free(h, &p); return fail(h, DVBS2HIP_EHIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e)); }
    h->bbf.all = p; h->bbf.bytes = bytes;
    for (int i = 0; i < 2; i++) { h->bbf.tx.p[i] = (int32_t *)(p + i * BBF_TX_STATE); h->bbf.rx.p[i] = (uint8_t *)(p + 2 * BBF_TX_STATE + i * rxb); }
    h->bbf.tx.cur = h->bbf.rx.cur = 0;
    h->bbf.ctr = (unsigned long long *)(p + 2 * BBF_TX_STATE + 2 * rxb);
    return 0;
}

// a workspace of the handle; inside a capture it has to be there already
static int bbf_ensure(dvbs2hip_t *h, int id, size_t bytes, void **out)
{
    if (h->capturing && h->bufs[id].bytes < bytes) return fail(h, DVBS2HIP_EINVAL, "run the sequence once before recording it: the first call of this size allocates its workspace");
    return ensure(h, id, bytes, out);
}

static int bbf_build_dev(dvbs2hip_t *h, const uint8_t *UP, int64_t n_bytes, int32_t *U_K, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!UP || !U_K) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if ((uintptr_t)U_K & 15) return fail(h, DVBS2HIP_EINVAL, "'U_K' has to be 16-byte aligned");
    const long long D = bbf_D(h);
    if (n_bytes <= (long long)(F - 1) * D || n_bytes > (long long)F * D)
        return fail(h, DVBS2HIP_EINVAL, "'n_bytes' has to be in ((n_frames - 1) D, n_frames D] with D = (K_bch - 80) / 8 = " + std::to_string(D) + " ('n_bytes' = " + std::to_string(n_bytes) +
                                            ", 'n_frames' = " + std::to_string(F) + ").");
    if ((r = bbf_state(h))) return r;
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, bbframe_build_launch(UP, n_bytes, U_K, h->bbf.tx.in(), h->bbf.tx.out(), bbf_params(h), F, h->stream));
    h->bbf.tx.flip();
    return 0;
}

static int bbf_parse_dev(dvbs2hip_t *h, const int32_t *V_K, const int8_t *VALID, uint8_t *UP, uint8_t *STATUS, int32_t *N_OUT, int32_t *HDR, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!V_K || !UP || !STATUS || !N_OUT) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if ((uintptr_t)V_K & 15) return fail(h, DVBS2HIP_EINVAL, "'V_K' has to be 16-byte aligned");
    if ((r = bbf_state(h))) return r;
    void *hdr, *plan;
    if ((r = bbf_ensure(h, B_BBF_HDRW, 32 * (size_t)F, &hdr)) || (r = bbf_ensure(h, B_BBF_PLAN, 16 * (size_t)F, &plan))) return r;
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, bbframe_parse_launch(V_K, VALID, (int32_t *)hdr, HDR, (int32_t *)plan, h->bbf.rx.in(), h->bbf.rx.out(), UP, STATUS, N_OUT, h->bbf.ctr, bbf_params(h), bbf_capacity(h, F), F,
                                   h->stream));
    h->bbf.rx.flip();
    return 0;
}

static int bbf_rx_bb_up_dev(dvbs2hip_t *h, const float *pl, const float *sigma, uint8_t *UP, uint8_t *STATUS, int32_t *N_OUT, int32_t *HDR, int8_t *cwd_l, int8_t *cwd_b, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    void *info, *c0 = cwd_l, *c1 = cwd_b;
    if ((r = bbf_ensure(h, B_INFO, (size_t)F * h->K_bch * 4, &info))) return r;
    if (!c0 && (r = bbf_ensure(h, B_CWD0, (size_t)F, &c0))) return r;
    if (!c1 && (r = bbf_ensure(h, B_CWD1, (size_t)F, &c1))) return r;
    if ((r = dvbs2hip_rx_bb_dev(h, pl, sigma, (int32_t *)info, (int8_t *)c0, (int8_t *)c1, F))) return r;
    return bbf_parse_dev(h, (const int32_t *)info, nullptr, UP, STATUS, N_OUT, HDR, F);
}

extern "C" {

int dvbs2hip_bbframe_set_params(dvbs2hip_t *h, int32_t matype1, int32_t matype2, int32_t upl_bits, int32_t sync, int32_t mark_tei)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "a capture is open on this handle");
    if (matype1 < 0 || matype1 > 255 || matype2 < 0 || matype2 > 255 || sync < 0 || sync > 255) return fail(h, DVBS2HIP_EINVAL, "'matype1', 'matype2' and 'sync' are bytes");
    if (upl_bits % 8 || upl_bits < 16 || upl_bits > h->K_bch - 80)
        return fail(h, DVBS2HIP_EUNSUPPORTED, "'upl_bits' has to be a multiple of 8 in [16, K_bch - 80] ('upl_bits' = " + std::to_string(upl_bits) + "): continuous streams are not provided");
    h->bbf.matype1 = matype1; h->bbf.matype2 = matype2; h->bbf.upl_bits = upl_bits; h->bbf.sync = sync; h->bbf.mark_tei = mark_tei ? 1 : 0;
    return dvbs2hip_bbframe_reset(h);
}

int dvbs2hip_bbframe_reset(dvbs2hip_t *h)
{
    int r = enter(h); if (r) return r;
    if (!h->bbf.all) return 0;
    HIPCHK(h, hipMemsetAsync(h->bbf.all, 0, h->bbf.bytes, h->stream));
    h->bbf.tx.cur = h->bbf.rx.cur = 0;
    return 0;
}

int dvbs2hip_bbframe_get_stats(dvbs2hip_t *h, uint64_t *stats)
{
    int r = enter(h); if (r) return r;
    if (!stats) return fail(h, DVBS2HIP_EINVAL, "null argument");
    memset(stats, 0, 5 * sizeof(uint64_t));
    if (!h->bbf.all) return 0;
    HIPCHK(h, hipMemcpyAsync(stats, h->bbf.ctr, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int dvbs2hip_bbframe_max_packets(dvbs2hip_t *h, int32_t F, int32_t *capacity)
{
    if (!h || !capacity) return DVBS2HIP_EINVAL;
    if (F < 1) return fail(h, DVBS2HIP_EINVAL, "'n_frames' has to be greater than 0");
    *capacity = bbf_capacity(h, F);
    return 0;
}

int dvbs2hip_bbframe_build_dev(dvbs2hip_t *h, const uint8_t *UP, int64_t n_bytes, int32_t *U_K, int32_t F) { return bbf_build_dev(h, UP, n_bytes, U_K, F); }

int dvbs2hip_bbframe_build(dvbs2hip_t *h, const uint8_t *UP, int64_t n_bytes, int32_t *U_K, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (n_bytes < 1) return fail(h, DVBS2HIP_EINVAL, "'n_bytes' has to be greater than 0");
    return host_call(h, F, false, {{UP, B_IN, (size_t)n_bytes}}, {{U_K, B_OUT, (size_t)F * h->K_bch * 4}},
                     [&](void *const *i, void *const *o, int nf) { return bbf_build_dev(h, (const uint8_t *)i[0], n_bytes, (int32_t *)o[0], nf); });
}

int dvbs2hip_bbframe_parse_dev(dvbs2hip_t *h, const int32_t *V_K, const int8_t *VALID, uint8_t *UP, uint8_t *STATUS, int32_t *N_OUT, int32_t *HDR, int32_t F)
{
    return bbf_parse_dev(h, V_K, VALID, UP, STATUS, N_OUT, HDR, F);
}

int dvbs2hip_bbframe_parse(dvbs2hip_t *h, const int32_t *V_K, const int8_t *VALID, uint8_t *UP, uint8_t *STATUS, int32_t *N_OUT, int32_t *HDR, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    const size_t cap = (size_t)bbf_capacity(h, F);
    return host_call(h, F, false, {{V_K, B_IN, (size_t)F * h->K_bch * 4}, {VALID, B_BBF_VALID, (size_t)F, 0, true}},
                     {{UP, B_BBF_UP, cap * (h->bbf.upl_bits / 8)}, {STATUS, B_BBF_STAT, cap}, {N_OUT, B_BBF_NOUT, 4}, {HDR, B_BBF_HDR, 32 * (size_t)F, 0, true}},
                     [&](void *const *i, void *const *o, int nf) {
                         return bbf_parse_dev(h, (const int32_t *)i[0], (const int8_t *)i[1], (uint8_t *)o[0], (uint8_t *)o[1], (int32_t *)o[2], HDR ? (int32_t *)o[3] : nullptr, nf);
                     });
}

int dvbs2hip_rx_bb_up_dev(dvbs2hip_t *h, const float *pl, const float *sigma, uint8_t *UP, uint8_t *STATUS, int32_t *N_OUT, int32_t *HDR, int8_t *cwd_l, int8_t *cwd_b, int32_t F)
{
    if (h && !pl) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    return bbf_rx_bb_up_dev(h, pl, sigma, UP, STATUS, N_OUT, HDR, cwd_l, cwd_b, F);
}

// what comes back is the packets, their statuses, the headers and the flags: K_bch / 8 bytes of a frame, not its 4 K_bch
int dvbs2hip_rx_bb_up(dvbs2hip_t *h, const float *pl, const float *sigma, uint8_t *UP, uint8_t *STATUS, int32_t *N_OUT, int32_t *HDR, int8_t *cwd_l, int8_t *cwd_b, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    const size_t cap = (size_t)bbf_capacity(h, F);
    return host_call(h, F, false, {{sigma, B_SIG, (size_t)F * 4, 0, true, true}, {pl, B_IN, (size_t)F * 2 * h->pl_frame * 4}},
                     {{UP, B_BBF_UP, cap * (h->bbf.upl_bits / 8)}, {STATUS, B_BBF_STAT, cap}, {N_OUT, B_BBF_NOUT, 4}, {HDR, B_BBF_HDR, 32 * (size_t)F, 0, true},
                      {cwd_l, B_CWD0, (size_t)F, 0, true}, {cwd_b, B_CWD1, (size_t)F, 0, true}},
                     [&](void *const *i, void *const *o, int nf) {
                         return bbf_rx_bb_up_dev(h, (const float *)i[1], (const float *)i[0], (uint8_t *)o[0], (uint8_t *)o[1], (int32_t *)o[2], HDR ? (int32_t *)o[3] : nullptr,
                                                 (int8_t *)o[4], (int8_t *)o[5], nf);
                     });
}

}  // extern "C"
