// C ABI, the PLHEADER walk (k_pls_walk.hip): from the header at `start` along the chain of PL frames whose lengths their own headers give, every frame's offset and
// value, and the frames grouped by value as pointer tables for the located decoders.  Stateless, and independent of the handle's MODCOD and max_frames; an extension
// with no reference task.
#include "dvbs2hip_handle.h"

using namespace dvbs2;

// the candidates start + 18 i that have a whole header in front of n_sym
static int plsw_candidates(int32_t n_sym, int32_t start) { return start + 90 <= n_sym ? (n_sym - 90 - start) / 18 + 1 : 0; }

// the shortest hop of the library's own table, in candidates; a caller's table may hold any multiple of 18 from 90 up
static int plsw_min_hop(bool callers_table)
{
    if (callers_table) return 90 / 18;
    static const int lib = [] {
        int m = 0;
        for (int v = 0; v < 256; v++) { const int L = dvbs2hip_pls_frame_symbols(v); if (L >= 90 && L % 18 == 0 && (!m || L < m)) m = L; }
        return m ? m / 18 : 90 / 18;
    }();
    return lib;
}

static int plsw_check(dvbs2hip_t *h, int32_t n_sym, int32_t start, int32_t max_out)
{
    int r = plss_check(h, n_sym); if (r) return r;
    if (start < 0 || start > n_sym) return fail(h, DVBS2HIP_EINVAL, "'start' has to be in [0, n_sym] ('start' = " + std::to_string(start) + ", 'n_sym' = " + std::to_string(n_sym) + ").");
    if (max_out < 1) return fail(h, DVBS2HIP_EINVAL, "'max_out' has to be at least 1 ('max_out' = " + std::to_string(max_out) + ").");
    return 0;
}

static int plsw_dev(dvbs2hip_t *h, const float *X, int32_t n_sym, int32_t start, const int32_t *LEN, float q_min, int32_t max_out, int32_t *OFF, int32_t *VAL, float *Q,
                    const float **SRC, int32_t *IDX, int32_t *CNT, int32_t *RES)
{
    int r = plsw_check(h, n_sym, start, max_out); if (r) return r;
    if (!X || !OFF || !VAL || !Q || !IDX || !CNT || !RES) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if ((uintptr_t)X & 7) return fail(h, DVBS2HIP_EINVAL, "'X' has to be 8-byte aligned");
    const int min_hop = plsw_min_hop(LEN != nullptr);
    if (!LEN && (r = plss_len(h, &LEN))) return r;
    const int M = plsw_candidates(n_sym, start), K = pls_walk_levels(M, min_hop, max_out);
    // the workspace is sized for start = 0, the most candidates and levels this n_sym and max_out can ask for: a recorded call needs one call of the same two before it
    const int M0 = plsw_candidates(n_sym, 0);
    void *work;
    if ((r = plss_ensure(h, B_PLSW_WORK, pls_walk_work_bytes(M0, pls_walk_levels(M0, min_hop, max_out)), &work))) return r;
    Timer tm(h, DVBS2HIP_K_MISC);
    if (M > 0) HIPCHK(h, pls_decode_launch(X + 2 * (size_t)start, nullptr, 18, (int32_t *)work, (float *)work + M, (float *)work + 2 * (size_t)M, M, h->stream));
    HIPCHK(h, pls_walk_launch(X, n_sym, start, M, K, pls_walk_choose(K), LEN, q_min, max_out, work, OFF, VAL, Q, SRC, IDX, CNT, RES, h->stream));
    return 0;
}

extern "C" {

int dvbs2hip_pls_walk_dev(dvbs2hip_t *h, const float *X, int32_t n_sym, int32_t start, const int32_t *LEN, float q_min, int32_t max_out, int32_t *OFF, int32_t *VAL,
                          float *Q, const float **SRC, int32_t *IDX, int32_t *CNT, int32_t *RES)
{
    return plsw_dev(h, X, n_sym, start, LEN, q_min, max_out, OFF, VAL, Q, SRC, IDX, CNT, RES);
}

int dvbs2hip_pls_walk(dvbs2hip_t *h, const float *X, int32_t n_sym, int32_t start, const int32_t *LEN, float q_min, int32_t max_out, int32_t *OFF, int32_t *VAL, float *Q,
                      int32_t *IDX, int32_t *CNT, int32_t *RES)
{
    int r = plsw_check(h, n_sym, start, max_out); if (r) return r;
    if (!X || !OFF || !VAL || !Q || !IDX || !CNT || !RES) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    // no walk writes more entries than the candidates hold frames
    const int M = plsw_candidates(n_sym, start);
    const size_t n = (size_t)std::min<long long>(max_out, M > 0 ? (M - 1) / (90 / 18) + 1 : 0);
    void *x, *len = nullptr, *out;
    if ((r = ensure(h, B_PLSS_X, 8 * (size_t)n_sym, &x)) || (r = ensure(h, B_PLSW_OUT, 4 * (4 * n + 256 + 4), &out)) || (LEN && (r = ensure(h, B_PLSS_LEN, 1024, &len)))) return r;
    int32_t *d_off = (int32_t *)out, *d_val = d_off + n, *d_idx = d_off + 3 * n, *d_cnt = d_off + 4 * n, *d_res = d_cnt + 256;
    float *d_q = (float *)out + 2 * n;
    HIPCHK(h, hipMemcpyAsync(x, X, 8 * (size_t)n_sym, hipMemcpyHostToDevice, h->stream));
    if (LEN) HIPCHK(h, hipMemcpyAsync(len, LEN, 1024, hipMemcpyHostToDevice, h->stream));
    if ((r = plsw_dev(h, (const float *)x, n_sym, start, (const int32_t *)len, q_min, max_out, d_off, d_val, d_q, nullptr, d_idx, d_cnt, d_res))) return r;
    if (n) {
        HIPCHK(h, hipMemcpyAsync(OFF, d_off, 4 * n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(VAL, d_val, 4 * n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(Q, d_q, 4 * n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(IDX, d_idx, 4 * n, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(CNT, d_cnt, 1024, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(RES, d_res, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
