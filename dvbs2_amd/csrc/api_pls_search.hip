// C ABI, the PLHEADER search (k_pls_search.hip): the PLS decoder at every symbol offset of a buffer, and the offset and value whose headers repeat at the frame length
// the value implies.  Stateless, and independent of the handle's MODCOD and max_frames; an extension with no reference task.
#include "dvbs2hip_handle.h"

using namespace dvbs2;

constexpr int32_t PLS_SCAN_MAX_SYM = DVBS2HIP_PLS_SCAN_MAX_SYM;      // the search's workspace is 12 bytes per offset: 192 MiB at the limit

namespace dvbs2 {

int plss_check(dvbs2hip_t *h, int32_t n_sym)
{
    int r = enter(h); if (r) return r;
    if (n_sym < 90 || n_sym > PLS_SCAN_MAX_SYM)
        return fail(h, DVBS2HIP_EINVAL, "'n_sym' has to be in [90, " + std::to_string(PLS_SCAN_MAX_SYM) + "] ('n_sym' = " + std::to_string(n_sym) + ").");
    return 0;
}

// a workspace of the handle; inside a capture it has to be there already
int plss_ensure(dvbs2hip_t *h, int id, size_t bytes, void **out)
{
    if (h->capturing && h->bufs[id].bytes < bytes) return fail(h, DVBS2HIP_EINVAL, "run the sequence once before recording it: the first call of this size allocates its workspace");
    return ensure(h, id, bytes, out);
}

static int plss_scan_dev(dvbs2hip_t *h, const float *X, int32_t n_sym, int32_t *PLS, float *MET, float *ENE)
{
    int r = plss_check(h, n_sym); if (r) return r;
    if (!X || !PLS) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if ((uintptr_t)X & 7) return fail(h, DVBS2HIP_EINVAL, "'X' has to be 8-byte aligned");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, pls_scan_launch(X, n_sym, PLS, MET, ENE, h->stream));
    return 0;
}

// the library's own table, on the device
int plss_len(dvbs2hip_t *h, const int32_t **LEN)
{
    if (!h->d_pls_len) {
        if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "run the sequence once before recording it: the first search with LEN = NULL uploads the library's table");
        int32_t t[256];
        for (int v = 0; v < 256; v++) t[v] = dvbs2hip_pls_frame_symbols(v);
        if (int r = upload(h, &h->d_pls_len, t, 256)) return r;
    }
    *LEN = h->d_pls_len;
    return 0;
}

}  // namespace dvbs2

static int plss_search_dev(dvbs2hip_t *h, const float *X, int32_t n_sym, const int32_t *LEN, int32_t *RES, float *SCORE)
{
    int r = plss_check(h, n_sym); if (r) return r;
    if (!X || !RES || !SCORE) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if ((uintptr_t)X & 7) return fail(h, DVBS2HIP_EINVAL, "'X' has to be 8-byte aligned");
    if (!LEN && (r = plss_len(h, &LEN))) return r;
    const size_t K = (size_t)n_sym - 89;
    void *out, *work;
    if ((r = plss_ensure(h, B_PLSS_OUT, 12 * K, &out)) || (r = plss_ensure(h, B_PLSS_WORK, pls_search_work_bytes(n_sym), &work))) return r;
    int32_t *pls = (int32_t *)out;
    float *met = (float *)out + K, *ene = (float *)out + 2 * K;
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, pls_scan_launch(X, n_sym, pls, met, ene, h->stream));
    HIPCHK(h, pls_search_launch(pls, met, ene, LEN, work, n_sym, RES, SCORE, h->stream));
    return 0;
}

extern "C" {

int dvbs2hip_pls_frame_symbols(int32_t value)
{
    return value >= 0 && value <= 255 && (value & 1) ? pl_frame_by_pls(value >> 1) : 0;
}

int dvbs2hip_pls_scan_dev(dvbs2hip_t *h, const float *X, int32_t n_sym, int32_t *PLS, float *MET, float *ENE) { return plss_scan_dev(h, X, n_sym, PLS, MET, ENE); }

int dvbs2hip_pls_scan(dvbs2hip_t *h, const float *X, int32_t n_sym, int32_t *PLS, float *MET, float *ENE)
{
    int r = plss_check(h, n_sym); if (r) return r;
    if (!X || !PLS) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    const size_t K = (size_t)n_sym - 89;
    void *x, *out;
    if ((r = ensure(h, B_PLSS_X, 8 * (size_t)n_sym, &x)) || (r = ensure(h, B_PLSS_OUT, 12 * K, &out))) return r;
    HIPCHK(h, hipMemcpyAsync(x, X, 8 * (size_t)n_sym, hipMemcpyHostToDevice, h->stream));
    int32_t *d_pls = (int32_t *)out;
    float *d_met = (float *)out + K, *d_ene = (float *)out + 2 * K;
    if ((r = plss_scan_dev(h, (const float *)x, n_sym, d_pls, MET ? d_met : nullptr, ENE ? d_ene : nullptr))) return r;
    HIPCHK(h, hipMemcpyAsync(PLS, d_pls, 4 * K, hipMemcpyDeviceToHost, h->stream));
    if (MET) HIPCHK(h, hipMemcpyAsync(MET, d_met, 4 * K, hipMemcpyDeviceToHost, h->stream));
    if (ENE) HIPCHK(h, hipMemcpyAsync(ENE, d_ene, 4 * K, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int dvbs2hip_pls_search_dev(dvbs2hip_t *h, const float *X, int32_t n_sym, const int32_t *LEN, int32_t *RES, float *SCORE) { return plss_search_dev(h, X, n_sym, LEN, RES, SCORE); }

int dvbs2hip_pls_search(dvbs2hip_t *h, const float *X, int32_t n_sym, const int32_t *LEN, int32_t *RES, float *SCORE)
{
    int r = plss_check(h, n_sym); if (r) return r;
    if (!X || !RES || !SCORE) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    void *x, *len = nullptr, *res;
    if ((r = ensure(h, B_PLSS_X, 8 * (size_t)n_sym, &x)) || (r = ensure(h, B_PLSS_RES, 32, &res)) || (LEN && (r = ensure(h, B_PLSS_LEN, 1024, &len)))) return r;
    HIPCHK(h, hipMemcpyAsync(x, X, 8 * (size_t)n_sym, hipMemcpyHostToDevice, h->stream));
    if (LEN) HIPCHK(h, hipMemcpyAsync(len, LEN, 1024, hipMemcpyHostToDevice, h->stream));
    if ((r = plss_search_dev(h, (const float *)x, n_sym, (const int32_t *)len, (int32_t *)res, (float *)res + 4))) return r;
    HIPCHK(h, hipMemcpyAsync(RES, res, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(SCORE, (float *)res + 4, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
