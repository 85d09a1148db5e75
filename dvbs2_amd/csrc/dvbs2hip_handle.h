// What the translation units of the C ABI share (dvbs2hip_api.hip and api_*.hip): the handle, its staging buffers and device allocations, the error plumbing and the
// host form of a task.  Private to the library's host side; the kernels' header is dvbs2hip_internal.h.
#pragma once
#include "dvbs2hip_internal.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <utility>

namespace dvbs2 {

extern thread_local std::string g_create_error;      // what dvbs2hip_last_error(NULL) returns (dvbs2hip_api.hip)

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

// state a task carries from call to call, in two device buffers: a call reads in(), writes out(), and flip()s once its launch is queued.  The buffers belong to the
// handle as before (dev_alloc / dev_free on p[i], or a part of a larger allocation); a reset makes buffer 0 the current one (cur = 0)
template <typename T>
struct PingPong {
    T *p[2] = {nullptr, nullptr};
    int cur = 0;
    T *in() const { return p[cur]; }
    T *out() const { return p[cur ^ 1]; }
    void flip() { cur ^= 1; }
};

}  // namespace dvbs2

struct dvbs2hip_handle {
    // configuration
    int N_ldpc = 0, K_ldpc = 0, K_bch = 0, bps = 0, itl_cols = 1, itl_order = 0;
    int n_sym = 0, pl_frame = 0, max_frames = 1, device = 0;
    int n_ite = 50, early_stop = 1, implem = 0;
    float alpha = 1.f, code_rate = 0.f;
    int fir_T = 0, fir_osf = 1;
    bool fir_sym = false;               // taps[i] == taps[T - 1 - i] for every i (what k_stepmf.hip's folded matched filter needs)
    // device state
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool capturing = false;
    bool lat_lds_ok = false;      // the device's LDS holds k_ldpc_lat.hip's image + state (gfx950: 160 KB)
    bool comm_dead = false;       // dvbs2hip_monitor_reduce timed out: the communicator was aborted
    int red_timeout_ms = 0;
    std::vector<hipGraphExec_t> graphs;      // dvbs2hip_graph_end: captured call sequences (a freed slot is nullptr)
    int n_cus = 256;
    dvbs2::LdpcPlan ldpc;
    dvbs2::BchPlan bch;
    float *d_cstl = nullptr;
    uint8_t *d_pl_seq = nullptr;
    float *d_taps_rev = nullptr;
    uint16_t *d_fir_afrag = nullptr, *d_upfir_afrag = nullptr;       // Toeplitz fragments of the split taps for the matrix-core FIR (T <= 81)
    dvbs2::PingPong<float> d_hist;   // the matched filter's memory at bw.S == 1 (dvbs2::bw_hist)
    void *d_hist_all = nullptr;      // one allocation behind d_hist and d_uphist
    size_t hist_stride = 0;
    float *d_taps = nullptr;            // natural order (shaping filter)
    dvbs2::PingPong<float> d_uphist;
    unsigned long long *d_ctr = nullptr;
    float *d_gwork = nullptr;
    // TX mirror (N1)
    uint32_t *d_enc_tab = nullptr;
    int32_t *d_enc_deg = nullptr;
    float *d_plh = nullptr;
    int pls_value = 0;                 // what the PLS decoder returns for a frame of this handle's own framer: cfg.pls as b0..b6, pilots = 1 (dvbs2hip_pls_expected)
    int32_t *d_pls_len = nullptr;      // PLHEADER search (api_pls_search.hip): dvbs2hip_pls_frame_symbols(0 .. 255), uploaded by the first search that passes LEN = NULL
    int enc_stride = 0;
    unsigned long long *d_bch_tab = nullptr, *d_bch_shift = nullptr;
    uint32_t *d_syn_pos = nullptr, *d_prbs_s = nullptr;     // (round 5) the LDPC kernel's BCH verification in the fused chain: row records + reduction table (LdpcKParams::syn_tab), PRBS words by (storage row, wave)
    int syn_words = 0, syn_rows = 0;
    std::map<int, dvbs2::DevBuf> bufs;        // lazily grown staging / intermediate buffers
    std::vector<void *> dev_owned;     // every other device allocation of the handle (dev_malloc / dev_free): what dvbs2hip_destroy frees
    // frame synchronizer (N4): device-resident state of Synchronizer_frame_DVBS2_fast
    struct {
        bool ready = false;
        float alpha = 0.9f, trigger = 30.f;    // factory defaults, Factory/Module/Synchronizer_frame/Synchronizer_frame.hpp:26-27
        int vec_width = 8;                     // mipp::N<float>() of the reference build (AVX2)
        int nbuff2 = 0;
        dvbs2::PingPong<float> xh;             // last 64 input samples (the correlators' memories + reg_channel)
        dvbs2::PingPong<float> sofh;           // last 64 cor_SOF samples (SOF_PLSC_delay)
        float *cv = nullptr;                   // corr_vec
        dvbs2::PingPong<float> buff2;          // output_delay.buff2 ...
        dvbs2::PingPong<int> st;               // ... and its {head2, first_time}: the two flip together
        dvbs2::PingPong<float> yprev;          // the last output frame of the previous call
        unsigned long long *keys = nullptr;    // arg max keys, max_frames x ceil(pl_frame / 64)
        float *metric = nullptr;               // max_corr of the last frame
        uint16_t *frag = nullptr;              // band fragments of the two correlators for the matrix cores (k_sync_mfma.hip)
        int n_alloc = 0;                       // streams the state above holds, side by side (dvbs2hip_set_streams; 1 without it)
    } sfm;
    // L&R fine frequency synchronizer (N4): damped autocorrelation R_l, alpha (factory default 0.999)
    // host sockets the integrator has pinned (dvbs2hip_host_register): base address -> bytes; copy streams + events of
    // the chunked host-form pipeline (H2D of chunk i+1 | kernels of chunk i | D2H of chunk i-1)
    std::map<uintptr_t, size_t> pinned;
    hipStream_t s_in = nullptr, s_out = nullptr;
    std::vector<hipEvent_t> ev_pipe;
    int ldpc_sched = DVBS2HIP_SCHED_QC;
    int sep = 0, sep_ax[2] = {0, 0};       // separable 2-bit constellation: linear exact LLRs (k_front.hip, demap_sep2)
    float sep_g[2] = {0.f, 0.f}, sep_h[2] = {0.f, 0.f};
    int fir_kernel = DVBS2HIP_FIR_AUTO;
    float *d_nat_work = nullptr;       // natural-order LDPC: frame-interleaved image + state, ceil(max_frames / 64) groups
    float *d_lr_R = nullptr;           // 2 floats per stream, lr_n streams
    int lr_n = 0;
    float lr_alpha = 0.999f;
    int lr_timeouts = 0;               // launches whose rotation had to be repeated (dvbs2hip_sync_lr_timeouts)
    // pilot-aided noise estimator (api_est_pilots.hip): the averaging factor and, once a call has run with alpha > 0, {Abar, Nbar, started} per stream (n_alloc streams)
    struct { float alpha = 0.f; float *st = nullptr; int n_alloc = 0; } estp;
    // BBFRAME layer (api_bbframe.hip): the parameters, and once a call has run the two tasks' states (ping-pong) and the five counters, one allocation: a reset is one memset
    struct {
        int matype1 = 0xF2, matype2 = 0, upl_bits = 1504, sync = 0x47, mark_tei = 0;
        void *all = nullptr;
        size_t bytes = 0;
        dvbs2::PingPong<int32_t> tx;
        dvbs2::PingPong<uint8_t> rx;
        unsigned long long *ctr = nullptr;
    } bbf;
    // L&R, recurrence and rotation in one launch (k_sync.hip, sff_lr_fused_kernel): the error word a rotating workgroup sets when it gives up waiting for the
    // recurrence -- host-mapped memory, so the host reads it at its synchronisation points without a copy
    // (round 5) every outstanding L&R call has its OWN error word and its OWN estimate buffer (LR_SLOTS in rotation): a later L&R or pilot-phase call
    // neither consumes an earlier call's error word nor overwrites the estimates its repair needs
    static constexpr int LR_SLOTS = 4;
    uint32_t *lr_err_host = nullptr, *lr_err_dev = nullptr;          // [LR_SLOTS]
    struct { const float *x = nullptr; float *y = nullptr; int n = 0, F = 0; bool pending = false; } lr_slot[LR_SLOTS];      // device-form calls not yet looked at: what dvbs2hip_synchronize re-rotates after a timeout
    int lr_next = 0;
    float *d_hist_zero = nullptr, *d_hist_junk = nullptr;     // filter2: zero history in, discarded history out
    // monitor reduction over RCCL (one process per GPU): communicator + the 3 x uint64 receive buffer
    void *nccl_comm = nullptr;
    unsigned long long *d_red = nullptr;
    unsigned long long *h_red = nullptr;      // pinned: the reduced counters' way back (a copy into pageable memory would wait for the stream itself -- and for a dead peer for ever)
    int red_rank = 0, red_world = 1;
    // timing
    // Synchronizer_freq_coarse_DVBS2_aib, one state per stream (SfcState: the PLL, Multiplier_sine_ccc_naive's nu in millionths and its sample counter n).  The loop
    // (k_stepmf.hip) runs on the device copy, the block-wise shift of the transmission phase (nco_kernel) takes nu and n as launch arguments from the host copy: `where`
    // says which of the two is current, and the side that is behind is brought up when it is next needed (one small copy at the switch between the phases)
    struct {
        enum { HOST = 0, DEV = 1, BOTH = 2 };
        int where = HOST;
        std::vector<dvbs2::SfcState> hs;                               // S entries
        std::vector<float> frq;                                 // what the shift task reports in FRQ: -nu after set_freq, estimated_freq after the loop
        int pll_sps = 1;                                        // Synchronizer_freq_coarse_DVBS2_aib.cpp:23 and Factory/Module/Synchronizer_freq_coarse/Synchronizer_freq_coarse.hpp:26-27
        float damping = 0.70710678f, nbw = 1e-4f;
        int n_alloc = 0;
        dvbs2::PingPong<dvbs2::SfcState> cf;
        dvbs2::PingPong<float> hist;                            // the matched filter's memory per stream while stm.S != bw.S (otherwise the loop runs on the block-wise filter's, dvbs2::bw_hist)
        bool hist_stale = false;                                // the streams started over: their matched-filter memories have to be cleared before the next loop call
        float *pil = nullptr;                                   // scrambled_pilots, n_p complex entries
        int n_p = 0;
        int smf_kernel = DVBS2HIP_SMF_LANE;                     // dvbs2hip_sync_step_mf_set_kernel: the loop's form, read at launch; no reset touches it
    } sfc;
    // symbol-timing recovery (Synchronizer_Gardner_fast_osf2): per-stream state and carry buffers in ping-pong pairs, like the filters' memories
    struct {
        float damping = 0.70710678f, nbw = 5e-5f, dg = 2.f;     // Factory/Module/Synchronizer_timing/Synchronizer_timing.hpp:28-30
        float kp = 0.f, ki = 0.f;
        int S = 1;                                              // streams per call (dvbs2hip_sync_timing_set_streams)
        int type = DVBS2HIP_STM_FAST, hold = 101;               // dvbs2hip_sync_timing_set_type: the loop and, for ULTRA, its hold size (--stm-hold-size)
        bool act = false;                                       // Synchronizer_timing::set_act: ULTRA holds only while it is set
        int Fs = 0;                                             // frames per stream of every call since the last reset (0: not yet fixed)
        int n_alloc = 0;                                        // streams the buffers below hold
        dvbs2::PingPong<dvbs2::StmState> st;
        dvbs2::PingPong<float> carry;                           // n_alloc x cap reals ...
        dvbs2::PingPong<int32_t> ccnt;                          // ... and the reals held per stream: the two flip together
        long long cap = 0;                                      // reals per stream
        int32_t *uf = nullptr;                                  // underflow counts per frame slot, max_frames
    } stm;
    // the channel's delay tasks: D, the Farrow taps of mu = D - floor(D), floor(D) + 1 samples of history (ping-pong)
    struct {
        float D = 2.f;
        float b[3] = {0.f, 1.f, 0.f};
        long long H = 3;
        dvbs2::PingPong<float> hist;
        float fs_omega = 0.f;                                   // the frequency shift: Multiplier_sine_ccc_naive's omega and sample counter
        uint32_t fs_n = 0;
    } chn;
    // dvbs2hip_set_streams: streams per call in the block-wise tasks that keep a memory (matched filter, frame synchronizer, L&R); the timing tasks' count is stm.S, and
    // dvbs2hip_sync_timing_set_streams sets that one alone.  S > 1: the matched filter's memory per stream, (fir_T - 1) complex samples each, side by side in a ping-pong pair
    // of its own (S = 1 stays on d_hist); dvbs2::bw_hist returns the pair of the current count, and the coarse-frequency loop runs on it too when stm.S == S (api_acquire.hip)
    struct {
        int S = 1;
        dvbs2::PingPong<float> hist;
        int hist_n = 0;                                         // streams hist holds
    } bw;
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[DVBS2HIP_K_COUNT];
    std::string err;
    std::string ldpc_name;
};

namespace dvbs2 {

inline int fail(dvbs2hip_t *h, int code, const std::string &msg)
{
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

#define HIPCHK(h, expr)                                                                              \
    do {                                                                                             \
        hipError_t e__ = (expr);                                                                     \
        if (e__ != hipSuccess)                                                                       \
            return dvbs2::fail(h, DVBS2HIP_EHIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

enum BufId { B_IN = 0, B_OUT, B_AUX0, B_AUX1, B_AUX2, B_AUX3, B_LLR, B_PACKED, B_EST, B_CWD0, B_CWD1, B_INFO, B_SIG, B_TXBCH, B_TXLDPC,
             B_SFM_CORR, B_SFM_MET, B_SFM_SOF, B_SFM_PLSC, B_SFM_DLY, B_SFM_DTAB, B_SFF_TMP, B_SFF_OUT, B_FLT2, B_MON_BE, B_MON_OUT, B_BCHFLAG, B_ORDER, B_LR_TMP0, B_LR_TMP1, B_LR_TMP2, B_LR_TMP3, B_SFM_SCR, B_SFM_NEED,
             B_STM_X, B_STM_Y, B_STM_B, B_STM_MU, B_STM_Y2, B_STM_UFW, B_STM_RDY, B_SMF_DEL, B_SMF_FRQ, B_PLS_HDR, B_PLS_OUT, B_ESTP_SYM, B_ESTP_OUT, B_ESTP_AN,
             B_BBF_UP, B_BBF_STAT, B_BBF_NOUT, B_BBF_HDR, B_BBF_HDRW, B_BBF_PLAN, B_BBF_VALID, B_PLSS_X, B_PLSS_OUT, B_PLSS_WORK, B_PLSS_LEN, B_PLSS_RES, B_PLSW_WORK, B_PLSW_OUT };

inline int ensure(dvbs2hip_t *h, int id, size_t bytes, void **out)
{
    DevBuf &b = h->bufs[id];
    if (b.bytes < bytes) {
        if (b.p) { HIPCHK(h, hipStreamSynchronize(h->stream)); HIPCHK(h, hipFree(b.p)); b.p = nullptr; b.bytes = 0; }
        hipError_t e = hipMalloc(&b.p, bytes);
        if (e != hipSuccess) return fail(h, DVBS2HIP_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
        b.bytes = bytes;
    }
    *out = b.p;
    return 0;
}

// ---- long-lived device memory: every allocation is entered in the handle's registry (dev_owned), and dvbs2hip_destroy frees what is still in it.  The caller
// synchronizes the stream before it frees a buffer that a kernel may still use.
template <typename T>
hipError_t dev_malloc(dvbs2hip_t *h, T **p, size_t bytes)
{
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes);
    if (e == hipSuccess) h->dev_owned.push_back(q);
    *p = (T *)q;                                     // (null after a failure)
    return e;
}
template <typename T>
int dev_alloc(dvbs2hip_t *h, T **p, size_t bytes, const std::string &what)
{
    return dev_malloc(h, p, bytes) == hipSuccess ? 0 : fail(h, DVBS2HIP_ENOMEM, what);
}
// the form of HIPCHK(h, hipMalloc(p, bytes)), code and text
#define DEV_ALLOC_CHK(h, p, bytes) \
    do { if (hipError_t e__ = dvbs2::dev_malloc(h, p, bytes)) return dvbs2::fail(h, DVBS2HIP_EHIP, std::string("hipMalloc((void **)" #p ", " #bytes "): ") + hipGetErrorString(e__)); } while (0)
template <typename T>
hipError_t dev_free(dvbs2hip_t *h, T **p)
{
    if (!*p) return hipSuccess;
    auto it = std::find(h->dev_owned.begin(), h->dev_owned.end(), (void *)*p);
    if (it != h->dev_owned.end()) { *it = h->dev_owned.back(); h->dev_owned.pop_back(); }
    const hipError_t e = hipFree((void *)*p);
    *p = nullptr;
    return e;
}
template <typename T>
int upload(dvbs2hip_t *h, T **dst, const T *src, size_t n)
{
    DEV_ALLOC_CHK(h, dst, n * sizeof(T));
    HIPCHK(h, hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
template <typename T>
int upload(dvbs2hip_t *h, T **dst, const std::vector<T> &src) { return upload(h, dst, src.data(), src.size()); }

// every entry point that touches HIP selects the handle's device first: a process may drive several GPUs, one handle each
inline int enter(dvbs2hip_t *h)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (hipSetDevice(h->device) != hipSuccess) return fail(h, DVBS2HIP_EHIP, "hipSetDevice failed");
    return 0;
}
inline int check_frames(dvbs2hip_t *h, int n_frames)
{
    int r0 = enter(h); if (r0) return r0;
    if (n_frames < 1 || n_frames > h->max_frames)
        return fail(h, DVBS2HIP_EINVAL, "'n_frames' has to be in [1, max_frames] ('n_frames' = " + std::to_string(n_frames) +
                                            ", 'max_frames' = " + std::to_string(h->max_frames) + ").");
    return 0;
}

// the block-wise tasks with a memory: stream s = frames [s F/S, (s+1) F/S) of a call (dvbs2hip_set_streams)
inline int bw_check(dvbs2hip_t *h, int n_frames)
{
    int r = check_frames(h, n_frames); if (r) return r;
    if (n_frames % h->bw.S)
        return fail(h, DVBS2HIP_EINVAL, "'n_frames' has to be a multiple of the stream count ('n_frames' = " + std::to_string(n_frames) + ", streams = " + std::to_string(h->bw.S) + ").");
    return 0;
}

// ---- host-socket pipeline for PINNED sockets: the batch goes through in chunks, copies on two copy streams (the two DMA
// directions run together), kernels on the handle's stream, so a call costs about max(H2D, D2H) instead of H2D + kernels + D2H
struct HostCopy { const void *src; void *dst; size_t bytes_per_frame; };       // H2D: src = host, dst = device; D2H: src = device, dst = host

inline bool host_is_pinned(const dvbs2hip_t *h, const void *p, size_t bytes)
{
    if (!p || h->pinned.empty()) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    auto it = h->pinned.upper_bound(a);
    if (it == h->pinned.begin()) return false;
    --it;
    return a >= it->first && a + bytes <= it->first + it->second;
}

template <typename Fn>
int host_pipeline(dvbs2hip_t *h, int F, const std::vector<HostCopy> &ins, const std::vector<HostCopy> &outs, Fn dev_call)
{
    const int n_chunks = F >= 1024 ? 8 : F >= 128 ? 4 : 1;
    const int chunk = (F + n_chunks - 1) / n_chunks;
    if (!h->s_in) { HIPCHK(h, hipStreamCreateWithFlags(&h->s_in, hipStreamNonBlocking)); HIPCHK(h, hipStreamCreateWithFlags(&h->s_out, hipStreamNonBlocking)); }
    while ((int)h->ev_pipe.size() < 2 * n_chunks) { hipEvent_t e; HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming)); h->ev_pipe.push_back(e); }
    HIPCHK(h, hipStreamSynchronize(h->stream));             // what the handle's stream still does with the staging buffers
    int c = 0;
    for (int f0 = 0; f0 < F; f0 += chunk, c++) {
        const int nf = F - f0 < chunk ? F - f0 : chunk;
        for (const HostCopy &x : ins)
            HIPCHK(h, hipMemcpyAsync((char *)x.dst + (size_t)f0 * x.bytes_per_frame, (const char *)x.src + (size_t)f0 * x.bytes_per_frame,
                                     (size_t)nf * x.bytes_per_frame, hipMemcpyHostToDevice, h->s_in));
        HIPCHK(h, hipEventRecord(h->ev_pipe[2 * c], h->s_in));
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_pipe[2 * c], 0));
        int r = dev_call(f0, nf);
        if (r) { (void)hipStreamSynchronize(h->s_in); (void)hipStreamSynchronize(h->stream); (void)hipStreamSynchronize(h->s_out); return r; }
        HIPCHK(h, hipEventRecord(h->ev_pipe[2 * c + 1], h->stream));
        HIPCHK(h, hipStreamWaitEvent(h->s_out, h->ev_pipe[2 * c + 1], 0));
        for (const HostCopy &x : outs)
            if (x.dst)
                HIPCHK(h, hipMemcpyAsync((char *)x.dst + (size_t)f0 * x.bytes_per_frame, (const char *)x.src + (size_t)f0 * x.bytes_per_frame,
                                         (size_t)nf * x.bytes_per_frame, hipMemcpyDeviceToHost, h->s_out));
    }
    HIPCHK(h, hipStreamSynchronize(h->s_out));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

struct Timer {      // RAII: events around one kernel launch when timing is on
    dvbs2hip_t *h; int k; hipEvent_t a = nullptr, b = nullptr;
    Timer(dvbs2hip_t *h_, int k_) : h(h_), k(k_)
    {
        if (!h->timing) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        (void)hipEventRecord(a, h->stream);
    }
    ~Timer()
    {
        if (!a) return;
        (void)hipEventRecord(b, h->stream);
        h->ev[k].push_back({a, b});
    }
};

// ---- the host form of a task: stage the host sockets in the handle's buffers, run the device form on them, copy the results back, wait.
struct HostSock {
    const void *host;      // the caller's socket (an output is written through it)
    int id;                // staging buffer; sockets that share one say where in it they start
    size_t bytes;          // of the whole call
    size_t off = 0;
    bool opt = false;      // may be null: a null input is not staged and the device form gets null; a null output is staged for the device form and not copied back
    bool whole = false;    // an input the pipeline does not split: copied once on the handle's stream, ahead of everything else; it need not be pinned
};
constexpr int HOST_SOCKS = 8;
// dev_call(in, out, n_frames) gets the sockets' device addresses in list order.  per_frame: the task treats frames independently or as one stream in order, so a call
// whose sockets are all pinned goes through in overlapped chunks (dev_call then runs once per chunk, on that chunk's part of every socket)
template <typename Fn>
int host_call(dvbs2hip_t *h, int F, bool per_frame, const std::vector<HostSock> &ins, const std::vector<HostSock> &outs, Fn dev_call)
{
    int r = check_frames(h, F); if (r) return r;
    for (const auto *v : {&ins, &outs}) for (const HostSock &s : *v) if (!s.host && !s.opt) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    void *din[HOST_SOCKS] = {}, *dout[HOST_SOCKS] = {};
    auto stage = [&](const HostSock &s, void **d) {
        size_t need = 0;                                                // a shared buffer is made for all its sockets at once (ensure may move it when it grows)
        for (const HostSock &t : ins) if (t.id == s.id && t.host) need = std::max(need, t.off + t.bytes);
        for (const HostSock &t : outs) if (t.id == s.id) need = std::max(need, t.off + t.bytes);
        void *p;
        if (int e = ensure(h, s.id, need, &p)) return e;
        *d = (char *)p + s.off;
        return 0;
    };
    bool pipe = per_frame;
    for (size_t i = 0; i < ins.size(); i++) {
        if (!ins[i].host) continue;
        if ((r = stage(ins[i], &din[i]))) return r;
        if (!ins[i].whole && !host_is_pinned(h, ins[i].host, ins[i].bytes)) pipe = false;
    }
    for (size_t i = 0; i < outs.size(); i++) {
        if ((r = stage(outs[i], &dout[i]))) return r;
        if (outs[i].host && !host_is_pinned(h, outs[i].host, outs[i].bytes)) pipe = false;
    }
    for (size_t i = 0; i < ins.size(); i++)
        if (ins[i].host && ins[i].whole) HIPCHK(h, hipMemcpyAsync(din[i], ins[i].host, ins[i].bytes, hipMemcpyHostToDevice, h->stream));
    if (pipe) {
        std::vector<HostCopy> ci, co;
        for (size_t i = 0; i < ins.size(); i++) if (ins[i].host && !ins[i].whole) ci.push_back({ins[i].host, din[i], ins[i].bytes / F});
        for (size_t i = 0; i < outs.size(); i++) co.push_back({dout[i], const_cast<void *>(outs[i].host), outs[i].bytes / F});
        return host_pipeline(h, F, ci, co, [&](int f0, int nf) {
            void *ci_f[HOST_SOCKS], *co_f[HOST_SOCKS];
            for (size_t i = 0; i < ins.size(); i++) ci_f[i] = din[i] ? (char *)din[i] + (size_t)f0 * (ins[i].bytes / F) : nullptr;
            for (size_t i = 0; i < outs.size(); i++) co_f[i] = (char *)dout[i] + (size_t)f0 * (outs[i].bytes / F);
            return dev_call(ci_f, co_f, nf);
        });
    }
    for (size_t i = 0; i < ins.size(); i++)
        if (ins[i].host && !ins[i].whole) HIPCHK(h, hipMemcpyAsync(din[i], ins[i].host, ins[i].bytes, hipMemcpyHostToDevice, h->stream));
    if ((r = dev_call(din, dout, F))) return r;
    for (size_t i = 0; i < outs.size(); i++)
        if (outs[i].host) HIPCHK(h, hipMemcpyAsync(const_cast<void *>(outs[i].host), dout[i], outs[i].bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// one socket in (B_IN), one socket out (B_OUT), with their element types
template <bool PER_FRAME = false, typename Tin, typename Tout, typename Fn>
int host_wrap(dvbs2hip_t *h, const Tin *in, size_t nin_el, Tout *out, size_t nout_el, int F, Fn dev_call)
{
    return host_call(h, F, PER_FRAME, {{in, B_IN, (size_t)F * nin_el * sizeof(Tin)}}, {{out, B_OUT, (size_t)F * nout_el * sizeof(Tout)}},
                     [&](void *const *i, void *const *o, int nf) { return dev_call((const Tin *)i[0], (Tout *)o[0], nf); });
}

// ---- defined in one translation unit, used from another
int lr_check_all(dvbs2hip_t *h);                                                   // api_sync.hip
int bw_hist(dvbs2hip_t *h, PingPong<float> **hist);                                // api_filter.hip: the block-wise matched filter's memory for bw.S streams -- d_hist at S = 1, bw.hist (allocated and cleared on first use) at S > 1
// api_tables.hip: what dvbs2hip_create uploads (pl_sequence: the coarse loop's pilots too)
struct TxEncTable { std::vector<uint32_t> tab; std::vector<int32_t> deg; int stride = 0; };
struct LdpcSynTables { std::vector<uint32_t> pos, prbs_s; int words = 0, rows = 0; };
void pl_sequence(std::vector<uint8_t> &seq);
std::vector<uint32_t> bb_prbs(int K);
std::vector<uint32_t> bb_prbs_by_row(const dvbs2hip_cfg &cfg, const std::vector<uint32_t> &prbs);
TxEncTable tx_enc_table(const dvbs2hip_cfg &cfg);
std::vector<unsigned long long> bch_byte_table(const std::vector<uint8_t> &gen);
std::vector<unsigned long long> bch_shift_table(const std::vector<uint8_t> &gen, int K_bch);
std::string ldpc_syn_tables(const dvbs2hip_cfg &cfg, const LdpcPlan &lp, const std::vector<uint8_t> &gen, const std::vector<uint32_t> &prbs, LdpcSynTables &t);
std::vector<float> plheader(const dvbs2hip_cfg &cfg);
const char *modcod_name_by_pls(int b0_b6);                                          // dvbs2hip_api.hip: the MODCOD of the library's table whose pls row is these seven bits (b0 the most significant), or null
int pl_frame_by_pls(int b0_b6);                                                     // dvbs2hip_api.hip: that MODCOD's PL frame in symbols, pilots on (the only frames the library builds), or 0
// api_pls_search.hip, for the search and the walk (api_pls_walk.hip): n_sym in [90, DVBS2HIP_PLS_SCAN_MAX_SYM]; a workspace of the handle, which inside a capture has
// to be there already; the library's own length table on the device (uploaded by the first call that asks for it, not inside a capture)
int plss_check(dvbs2hip_t *h, int32_t n_sym);
int plss_ensure(dvbs2hip_t *h, int id, size_t bytes, void **out);
int plss_len(dvbs2hip_t *h, const int32_t **LEN);
std::vector<float> unit_constellation(const dvbs2hip_cfg &cfg);
bool separable_2bit(const std::vector<float> &cs, int ax[2], float g[2], float hh[2]);

}  // namespace dvbs2
