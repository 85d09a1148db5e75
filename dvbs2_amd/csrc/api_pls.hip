// C ABI, the PLS decoder (k_pls.hip): the PLHEADER of aligned PL frames read back to the value the transmitter's framer encoded.  Stateless; an extension with no
// reference task.
#include "dvbs2hip_handle.h"

using namespace dvbs2;

// X_N1 with `stride` complex samples from frame to frame, or the located table SRC
static int pls_dev(dvbs2hip_t *h, const float *X_N1, const float *const *SRC, size_t stride, int32_t *PLS, float *MET, float *ENE, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if ((!X_N1 && !SRC) || !PLS) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, pls_decode_launch(X_N1, SRC, stride, PLS, MET, ENE, F, h->stream));
    return 0;
}

extern "C" {

int dvbs2hip_pls_decode_dev(dvbs2hip_t *h, const float *X_N1, int32_t *PLS, float *MET, float *ENE, int32_t F)
{
    return pls_dev(h, X_N1, nullptr, h ? (size_t)h->pl_frame : 0, PLS, MET, ENE, F);
}

int dvbs2hip_pls_decode_located_dev(dvbs2hip_t *h, const float *const *SRC, int32_t *PLS, float *MET, float *ENE, int32_t F)
{
    return pls_dev(h, nullptr, SRC, 0, PLS, MET, ENE, F);
}

// the host form stages the 90 header symbols of every frame and nothing else: 720 bytes of a frame of 27 to 266 KB
int dvbs2hip_pls_decode(dvbs2hip_t *h, const float *X_N1, int32_t *PLS, float *MET, float *ENE, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X_N1 || !PLS) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    const size_t hb = sizeof(float) * 2 * 90, nf4 = 4 * (size_t)F;
    void *hdr, *out;
    if ((r = ensure(h, B_PLS_HDR, hb * (size_t)F, &hdr)) || (r = ensure(h, B_PLS_OUT, 3 * nf4, &out))) return r;
    HIPCHK(h, hipMemcpy2DAsync(hdr, hb, X_N1, sizeof(float) * 2 * (size_t)h->pl_frame, hb, (size_t)F, hipMemcpyHostToDevice, h->stream));
    int32_t *d_pls = (int32_t *)out;
    float *d_met = (float *)out + F, *d_ene = (float *)out + 2 * (size_t)F;
    if ((r = pls_dev(h, (const float *)hdr, nullptr, 90, d_pls, MET ? d_met : nullptr, ENE ? d_ene : nullptr, F))) return r;
    HIPCHK(h, hipMemcpyAsync(PLS, d_pls, nf4, hipMemcpyDeviceToHost, h->stream));
    if (MET) HIPCHK(h, hipMemcpyAsync(MET, d_met, nf4, hipMemcpyDeviceToHost, h->stream));
    if (ENE) HIPCHK(h, hipMemcpyAsync(ENE, d_ene, nf4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int dvbs2hip_pls_expected(dvbs2hip_t *h, int32_t *value)
{
    if (!h || !value) return DVBS2HIP_EINVAL;
    *value = h->pls_value;
    return 0;
}

int dvbs2hip_pls_describe(int32_t value, char *name, int32_t name_len, int32_t *pilots)
{
    if (value < 0 || value > 255 || !name || name_len < 1) return DVBS2HIP_EINVAL;
    const char *n = modcod_name_by_pls(value >> 1);
    snprintf(name, (size_t)name_len, "%s", n ? n : "");
    if (pilots) *pilots = value & 1;
    return DVBS2HIP_OK;
}

}  // extern "C"
