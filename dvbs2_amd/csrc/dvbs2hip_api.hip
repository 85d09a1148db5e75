// C ABI of libdvbs2hip.so (include/dvbs2hip.h), first part: the handle's life (create / destroy, stream, graphs, pinned host memory, timers, memory helpers) and
// the FEC chain (LDPC, BCH, demodulator, deinterleaver, estimator, descramblers, the fused rx_bb / tx_bb).  The other tasks' entry points are in api_filter.hip,
// api_sync.hip, api_acquire.hip and api_monitor.hip, the tables created here are built in api_tables.hip, what they all share is dvbs2hip_handle.h.
// The arithmetic is in the k_*.hip files (docs/kernels.md).  No CPU fallback.
#include "dvbs2hip_handle.h"
#include "ldpc_dispatch.h"
#include "dvbs2_tables_gen.h"
#include <climits>
#include <new>

using namespace dvbs2;

namespace dvbs2 {
thread_local std::string g_create_error;

const char *modcod_name_by_pls(int b0_b6)
{
    for (int i = 0; i < DVBS2_N_MODCODS; i++) {
        int v = 0;
        for (int k = 0; k < 7; k++) v = v << 1 | (dvbs2_modcod_rows[i].pls[k] & 1);
        if (v == b0_b6) return dvbs2_modcod_rows[i].name;
    }
    return nullptr;
}

int pl_frame_by_pls(int b0_b6)
{
    for (int i = 0; i < DVBS2_N_MODCODS; i++) {
        const dvbs2_modcod_row &r = dvbs2_modcod_rows[i];
        int v = 0;
        for (int k = 0; k < 7; k++) v = v << 1 | (r.pls[k] & 1);
        const int n_sym = r.N_ldpc / r.bps;
        if (v == b0_b6) return 90 * (n_sym / 90 + 1) + (n_sym / (16 * 90)) * 36;         // DVBS2.cpp:351-355, as dvbs2hip_create
    }
    return 0;
}
}

extern "C" {

int dvbs2hip_cfg_from_modcod(const char *modcod, dvbs2hip_cfg *cfg)
{
    if (!cfg) return DVBS2HIP_EINVAL;
    std::string name = modcod ? modcod : "";
    if (name.empty()) name = "QPSK-S_8/9";
    for (int i = 0; i < DVBS2_N_MODCODS; i++) {
        const dvbs2_modcod_row &r = dvbs2_modcod_rows[i];
        if (name != r.name) continue;
        memset(cfg, 0, sizeof *cfg);
        cfg->N_ldpc = r.N_ldpc; cfg->K_ldpc = r.K_ldpc; cfg->K_bch = r.K_bch;
        cfg->ldpc_n_rows = r.ldpc_n_rows; cfg->ldpc_row_ptr = r.rp; cfg->ldpc_addr = r.ad;
        cfg->ldpc_n_ite = 50; cfg->ldpc_implem = DVBS2HIP_IMPLEM_SPA; cfg->ldpc_alpha = 1.0f; cfg->ldpc_early_stop = 1;
        cfg->bch_m = r.bch_m; cfg->bch_t = r.bch_t; cfg->bch_prim = r.prim;
        cfg->bps = r.bps; cfg->cstl = r.cstl;
        cfg->itl_cols = r.itl_cols; cfg->itl_order = r.itl_order;
        cfg->fir_n_taps = 81; cfg->fir_taps = rrc_taps_81; cfg->fir_osf = 2;
        cfg->max_frames = 1; cfg->device = 0; cfg->stream = nullptr; cfg->ldpc_lds_groups = -1;
        for (int k = 0; k < 7; k++) cfg->pls[k] = r.pls[k];
        return DVBS2HIP_OK;
    }
    g_create_error = name + " mod-cod scheme not supported.";
    return DVBS2HIP_EINVAL;
}

int dvbs2hip_device_count(int32_t *count)
{
    if (!count) return DVBS2HIP_EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return 0;
}

// everything dvbs2hip_create puts on the device, table by table: build on the host (api_tables.hip), upload.  An error is left in the handle, which the caller destroys
static int create_init(dvbs2hip_t *h, const dvbs2hip_cfg *cfg)
{
    int r;
    h->device = cfg->device;
    HIPCHK(h, hipSetDevice(h->device));
    hipDeviceProp_t prop;
    HIPCHK(h, hipGetDeviceProperties(&prop, h->device));
    h->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (cfg->stream) { h->stream = (hipStream_t)cfg->stream; h->own_stream = false; }
    else { HIPCHK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)); h->own_stream = true; }

    h->N_ldpc = cfg->N_ldpc; h->K_ldpc = cfg->K_ldpc; h->K_bch = cfg->K_bch; h->bps = cfg->bps;
    h->itl_cols = cfg->itl_cols; h->itl_order = cfg->itl_order; h->max_frames = cfg->max_frames;
    h->n_sym = cfg->N_ldpc / cfg->bps;
    h->pl_frame = 90 * (h->n_sym / 90 + 1) + (h->n_sym / (16 * 90)) * 36;      // DVBS2.cpp:351-355
    h->n_ite = cfg->ldpc_n_ite; h->early_stop = cfg->ldpc_early_stop ? 1 : 0; h->implem = cfg->ldpc_implem;
    h->alpha = cfg->ldpc_implem == DVBS2HIP_IMPLEM_MS ? 1.0f : cfg->ldpc_alpha;
    h->code_rate = (float)cfg->K_bch / (float)cfg->N_ldpc;                      // TX_RX_BB/main.cpp:142
    if (h->n_sym % 90) return fail(h, DVBS2HIP_EINVAL, "'N_ldpc / bps' has to be a multiple of the 90-symbol slot");

    // ---- LDPC
    // gfx950: a workgroup may own the CU's whole 160 KiB LDS (MI355X_MICROARCH "LDS")
    size_t lds_limit = strstr(prop.gcnArchName, "gfx950") ? 160 * 1024 : prop.sharedMemPerBlock;
    if (const char *ev = getenv("DVBS2HIP_LDS_LIMIT")) lds_limit = (size_t)atol(ev);
    if (lds_limit < 32 * 1024) lds_limit = 32 * 1024;
    h->lat_lds_ok = lds_limit >= 160 * 1024;
    lds_limit -= 512;                                    // static LDS of the kernel + slack
    LdpcPlan &lp = h->ldpc;
    std::string e = ldpc_build_plan(lp, cfg->N_ldpc, cfg->K_ldpc, cfg->ldpc_n_rows, cfg->ldpc_row_ptr, cfg->ldpc_addr,
                                    cfg->ldpc_lds_groups, lds_limit, cfg->ldpc_implem == DVBS2HIP_IMPLEM_SPA ? 3 : cfg->ldpc_implem == DVBS2HIP_IMPLEM_SPA_TANH ? 2 : cfg->ldpc_implem == DVBS2HIP_IMPLEM_SPA_EXACT ? 1 : 0, cfg->max_frames <= h->n_cus);
    if (!e.empty()) return fail(h, DVBS2HIP_EINVAL, e);
    if ((r = upload(h, &lp.d_entries, lp.entries)) || (r = upload(h, &lp.d_layer_deg, lp.layer_deg)) || (r = upload(h, &lp.d_layer_lvl, lp.layer_lvl)) || (r = upload(h, &lp.d_groups, lp.groups))) return r;
    if (lp.fast_wg8) {
        if ((r = upload(h, &lp.d_w8_tab, lp.w8_tab)) || (r = upload(h, &lp.d_w8_rows, lp.w8_rows))) return r;
        if (!lp.w8_atab.empty() && (r = upload(h, &lp.d_w8_atab, lp.w8_atab))) return r;
        DEV_ALLOC_CHK(h, &lp.d_cu_ctr, (LDPC_CU_CTR_WORDS + LDPC_PROF_WORDS) * sizeof(uint32_t));
        HIPCHK(h, hipMemset(lp.d_cu_ctr, 0, LDPC_CU_CTR_WORDS * sizeof(uint32_t)));
    }
    // the persistent grid and the tables of the fused chain are those of the kernel that large batches run on
    const LdpcChoice big = ldpc_choose(lp, {DVBS2HIP_SCHED_QC, INT_MAX, h->n_cus, h->lat_lds_ok, false, false});
    if (!big.error.empty()) return fail(h, DVBS2HIP_EUNSUPPORTED, big.error);
    lp.grid_max = ldpc_blocks_per_cu(lp, big) * h->n_cus;
    lp.n_cus = h->n_cus;
    if (const char *ev = getenv("DVBS2HIP_LDPC_GRID_MAX")) { const int g = atoi(ev); if (g >= 1 && g < lp.grid_max) lp.grid_max = g; }   // scaling experiments
    if (lp.gwork_words > 0) DEV_ALLOC_CHK(h, &h->d_gwork, (size_t)lp.grid_max * lp.gwork_words * sizeof(float));

    // ---- BCH, and the BB scrambler's sequence in the two orders its readers want
    e = bch_build_plan(h->bch, cfg->bch_m, cfg->bch_prim, cfg->bch_t, cfg->K_ldpc, cfg->K_bch);
    if (!e.empty()) return fail(h, DVBS2HIP_EINVAL, e);
    if ((r = upload(h, &h->bch.d_exp, h->bch.exp_)) || (r = upload(h, &h->bch.d_log, h->bch.log_)) || (r = upload(h, &h->bch.d_syn_tab, h->bch.syn_tab))) return r;
    const std::vector<uint32_t> prbs = bb_prbs(cfg->K_bch);
    if ((r = upload(h, &h->bch.d_prbs_rw, bb_prbs_by_row(*cfg, prbs))) || (r = upload(h, &h->bch.d_prbs, prbs))) return r;

    // ---- TX mirror tables: encoder layer table, BCH generator, PLHEADER
    const TxEncTable enc = tx_enc_table(*cfg);
    h->enc_stride = enc.stride;
    if ((r = upload(h, &h->d_enc_tab, enc.tab)) || (r = upload(h, &h->d_enc_deg, enc.deg))) return r;
    const std::vector<uint8_t> g = bch_generator(h->bch);
    if ((int)g.size() - 1 != cfg->K_ldpc - cfg->K_bch || g.size() > 193) return fail(h, DVBS2HIP_EINVAL, "BCH generator degree does not match N_bch - K_bch");
    if ((r = upload(h, &h->d_bch_tab, bch_byte_table(g))) || (r = upload(h, &h->d_bch_shift, bch_shift_table(g, h->K_bch)))) return r;
    if (big.family == LF_WG8) {       // the LDPC kernel's BCH verification in the fused chain
        LdpcSynTables syn;
        e = ldpc_syn_tables(*cfg, lp, g, prbs, syn);
        if (!e.empty()) return fail(h, DVBS2HIP_EINVAL, e);
        if ((r = upload(h, &h->d_syn_pos, syn.pos)) || (r = upload(h, &h->d_prbs_s, syn.prbs_s))) return r;
        h->syn_words = syn.words; h->syn_rows = syn.rows;
    }
    if ((r = upload(h, &h->d_plh, plheader(*cfg)))) return r;
    h->pls_value = 1;                                                              // (the framer's pairing is always the complementary one)
    for (int k = 0; k < 7; k++) h->pls_value |= (cfg->pls[k] & 1) << (7 - k);

    // ---- modem
    const std::vector<float> cs = unit_constellation(*cfg);
    if (cs.empty()) return fail(h, DVBS2HIP_EINVAL, "constellation has zero energy");
    if ((r = upload(h, &h->d_cstl, cs))) return r;
    if (cfg->bps == 2 && !getenv("DVBS2HIP_DEMAP_GENERAL")) {
        int ax[2]; float sg[2], sh[2];
        if (separable_2bit(cs, ax, sg, sh)) { h->sep = 1; for (int b = 0; b < 2; b++) { h->sep_ax[b] = ax[b]; h->sep_g[b] = sg[b]; h->sep_h[b] = sh[b]; } }
    }
    std::vector<uint8_t> seq;
    pl_sequence(seq);
    if (h->pl_frame - 90 > (int)seq.size()) return fail(h, DVBS2HIP_EINVAL, "PL frame longer than the scrambling sequence");
    if ((r = upload(h, &h->d_pl_seq, seq))) return r;

    // ---- matched filter: taps stored reversed (Filter_FIR_ccr.cpp:26-27)
    h->fir_T = cfg->fir_n_taps; h->fir_osf = cfg->fir_osf > 0 ? cfg->fir_osf : 1;
    if (h->fir_T > 0) {
        std::vector<float> rev(h->fir_T);
        for (int i = 0; i < h->fir_T; i++) rev[i] = cfg->fir_taps[h->fir_T - 1 - i];
        h->fir_sym = true;
        for (int i = 0; i < h->fir_T; i++) if (rev[i] != cfg->fir_taps[i]) h->fir_sym = false;
        if ((r = upload(h, &h->d_taps_rev, rev))) return r;
        if (h->fir_T <= 81 && (r = upload(h, &h->d_fir_afrag, fir_mfma_afrag(rev.data(), h->fir_T)))) return r;
        const size_t hb = sizeof(float) * 2 * (size_t)(h->fir_T > 1 ? h->fir_T - 1 : 1);
        // the four history buffers in ONE allocation, [hist 0 | uphist 0 | hist 1 | uphist 1]: dvbs2hip_filter_reset is then one memset of the first two (it makes them the current
        // ones) instead of four fill kernels -- ~50 us of the 250 us a one-frame call sequence takes (tools/r05_latency_trace.sh)
        h->hist_stride = (hb + 255) / 256 * 256;
        DEV_ALLOC_CHK(h, &h->d_hist_all, 4 * h->hist_stride);
        HIPCHK(h, hipMemset(h->d_hist_all, 0, 4 * h->hist_stride));
        for (int i = 0; i < 2; i++) { h->d_hist.p[i] = (float *)((char *)h->d_hist_all + (size_t)(2 * i) * h->hist_stride); h->d_uphist.p[i] = (float *)((char *)h->d_hist_all + (size_t)(2 * i + 1) * h->hist_stride); }
        if ((r = upload(h, &h->d_taps, cfg->fir_taps, (size_t)h->fir_T))) return r;
        if (h->fir_osf == 2) {
            const std::vector<uint16_t> af2 = upfir_mfma_afrag(cfg->fir_taps, h->fir_T);
            if (!af2.empty() && (r = upload(h, &h->d_upfir_afrag, af2))) return r;
        }
    }
    DEV_ALLOC_CHK(h, &h->d_ctr, 3 * sizeof(unsigned long long));
    HIPCHK(h, hipMemset(h->d_ctr, 0, 3 * sizeof(unsigned long long)));
    HIPCHK(h, hipDeviceSynchronize());
    return 0;
}

int dvbs2hip_create(const dvbs2hip_cfg *cfg, dvbs2hip_t **out)
{
    if (!cfg || !out) return fail(nullptr, DVBS2HIP_EINVAL, "null argument");
    *out = nullptr;
    if (cfg->max_frames < 1) return fail(nullptr, DVBS2HIP_EINVAL, "'max_frames' has to be greater than 0");
    if (cfg->max_frames > 65534) return fail(nullptr, DVBS2HIP_EINVAL, "'max_frames' has to be at most 65534 (frames are the second grid dimension of several kernels)");
    if (cfg->bps < 1 || cfg->bps > 5 || !cfg->cstl) return fail(nullptr, DVBS2HIP_EINVAL, "'bps' has to be in [1,5] with a constellation");
    if (cfg->N_ldpc <= 0 || cfg->N_ldpc % cfg->bps) return fail(nullptr, DVBS2HIP_EINVAL, "'N_ldpc' has to be a positive multiple of 'bps'");
    if (cfg->itl_cols > 1 && cfg->N_ldpc % cfg->itl_cols) return fail(nullptr, DVBS2HIP_EINVAL, "'N_ldpc' has to be a multiple of 'itl_cols'");
    if (cfg->ldpc_implem != DVBS2HIP_IMPLEM_NMS && cfg->ldpc_implem != DVBS2HIP_IMPLEM_MS && cfg->ldpc_implem != DVBS2HIP_IMPLEM_SPA && cfg->ldpc_implem != DVBS2HIP_IMPLEM_SPA_TANH && cfg->ldpc_implem != DVBS2HIP_IMPLEM_SPA_EXACT)
        return fail(nullptr, DVBS2HIP_EUNSUPPORTED, "LDPC implem not supported (NMS, MS, SPA, SPA_TANH and SPA_EXACT only)");
    if (!cfg->ldpc_row_ptr || !cfg->ldpc_addr || !cfg->bch_prim) return fail(nullptr, DVBS2HIP_EINVAL, "missing code tables");
    if (cfg->ldpc_n_ite < 1) return fail(nullptr, DVBS2HIP_EINVAL, "'ldpc_n_ite' has to be greater than 0");
    if (cfg->fir_n_taps < 0 || cfg->fir_n_taps > 257 || (cfg->fir_n_taps > 0 && !cfg->fir_taps))
        return fail(nullptr, DVBS2HIP_EINVAL, "'fir_n_taps' has to be in [0,257] with taps");

    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1)
        return fail(nullptr, DVBS2HIP_ENODEVICE, "no HIP device available (libdvbs2hip has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= n_dev) return fail(nullptr, DVBS2HIP_EINVAL, "'device' out of range");

    dvbs2hip_t *h = new (std::nothrow) dvbs2hip_handle;
    if (!h) return fail(nullptr, DVBS2HIP_ENOMEM, "out of host memory");
    if (const int r = create_init(h, cfg)) {
        const std::string msg = h->err;
        dvbs2hip_destroy(h);
        return fail(nullptr, r, msg);
    }
    *out = h;
    return DVBS2HIP_OK;
}

void dvbs2hip_destroy(dvbs2hip_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream && !h->comm_dead) (void)hipStreamSynchronize(h->stream);      // (a stream behind an aborted all-reduce may never drain)
    (void)dvbs2hip_monitor_reduce_finalize(h);
    for (hipGraphExec_t g : h->graphs) if (g) (void)hipGraphExecDestroy(g);
    for (auto &kv : h->bufs) if (kv.second.p) (void)hipFree(kv.second.p);
    for (int k = 0; k < DVBS2HIP_K_COUNT; k++)
        for (auto &p : h->ev[k]) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (auto &kv : h->pinned) (void)hipHostUnregister(reinterpret_cast<void *>(kv.first));
    for (hipEvent_t e : h->ev_pipe) (void)hipEventDestroy(e);
    if (h->s_in) (void)hipStreamDestroy(h->s_in);
    if (h->s_out) (void)hipStreamDestroy(h->s_out);
    for (void *p : h->dev_owned) (void)hipFree(p);
    if (h->lr_err_host) (void)hipHostFree(h->lr_err_host);
    if (h->h_red) (void)hipHostFree(h->h_red);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

const char *dvbs2hip_last_error(const dvbs2hip_t *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int dvbs2hip_set_ldpc_schedule(dvbs2hip_t *h, int32_t schedule)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (schedule != DVBS2HIP_SCHED_QC && schedule != DVBS2HIP_SCHED_NATURAL) return fail(h, DVBS2HIP_EINVAL, "unknown LDPC schedule");
    if (schedule == DVBS2HIP_SCHED_NATURAL && !h->ldpc.fast)
        return fail(h, DVBS2HIP_EUNSUPPORTED, "the natural-order schedule is implemented for codes with check degree <= 27");
    h->ldpc_sched = schedule;
    return 0;
}

// the kernel of a call of F frames on this handle, as the handle stands
static LdpcChoice ldpc_choice(const dvbs2hip_t *h, int F) { return ldpc_choose(h->ldpc, {h->ldpc_sched, F, h->n_cus, h->lat_lds_ok, h->early_stop != 0, h->d_syn_pos != nullptr}); }

const char *dvbs2hip_ldpc_kernel_name(const dvbs2hip_t *h)
{
    if (!h) return "";
    const_cast<dvbs2hip_t *>(h)->ldpc_name = ldpc_choice_name(ldpc_choice(h, h->max_frames));      // (the small-batch kernel where every call of this handle is a small batch)
    return h->ldpc_name.c_str();
}

int dvbs2hip_reset(dvbs2hip_t *h)
{
    if (!h) return DVBS2HIP_EINVAL;
    int r = dvbs2hip_filter_reset(h);
    if (r) return r;
    if ((r = dvbs2hip_estimate_pilots_reset(h))) return r;
    if ((r = dvbs2hip_bbframe_reset(h))) return r;
    return dvbs2hip_monitor_reset(h);
}

int dvbs2hip_set_ldpc_params(dvbs2hip_t *h, int32_t n_ite, float alpha, int32_t early_stop)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (n_ite < 1) return fail(h, DVBS2HIP_EINVAL, "'n_ite' has to be greater than 0");
    if (!(alpha > 0.f)) return fail(h, DVBS2HIP_EINVAL, "'alpha' has to be greater than 0");
    h->n_ite = n_ite; h->alpha = alpha; h->early_stop = early_stop ? 1 : 0;
    return 0;
}

void *dvbs2hip_get_stream(dvbs2hip_t *h) { return h ? (void *)h->stream : nullptr; }

int dvbs2hip_synchronize(dvbs2hip_t *h)
{
    int r0 = enter(h); if (r0) return r0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return lr_check_all(h);      // (device-form L&R calls: their error words are looked at here)
}

// ------------------------------------------------------------------ call sequences as hipGraphs (small batches: the sequence filter -> extract -> rx_bb is six launches
// and a fill for one workgroup's worth of work; captured once per (F, buffers) and replayed it is ONE submission)
int dvbs2hip_graph_begin(dvbs2hip_t *h)
{
    int r0 = enter(h); if (r0) return r0;
    if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "a capture is already open on this handle");
    if (h->timing) return fail(h, DVBS2HIP_EINVAL, "the per-kernel timers are on: their events cannot be recorded into a graph (dvbs2hip_timing_enable(h, 0) first)");
    HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    h->capturing = true;
    return 0;
}

int dvbs2hip_graph_end(dvbs2hip_t *h, int32_t *graph)
{
    if (!h || !graph) return DVBS2HIP_EINVAL;
    if (!h->capturing) return fail(h, DVBS2HIP_EINVAL, "no capture is open on this handle");
    h->capturing = false;
    hipGraph_t g = nullptr;
    HIPCHK(h, hipStreamEndCapture(h->stream, &g));
    hipGraphExec_t ex = nullptr;
    hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIPCHK(h, e);
    size_t k = 0;
    while (k < h->graphs.size() && h->graphs[k]) k++;
    if (k == h->graphs.size()) h->graphs.push_back(ex); else h->graphs[k] = ex;
    *graph = (int32_t)k;
    return 0;
}

int dvbs2hip_graph_launch(dvbs2hip_t *h, int32_t graph)
{
    int r0 = enter(h); if (r0) return r0;
    if (graph < 0 || (size_t)graph >= h->graphs.size() || !h->graphs[(size_t)graph]) return fail(h, DVBS2HIP_EINVAL, "unknown graph");
    HIPCHK(h, hipGraphLaunch(h->graphs[(size_t)graph], h->stream));
    return 0;
}

int dvbs2hip_graph_destroy(dvbs2hip_t *h, int32_t graph)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (graph < 0 || (size_t)graph >= h->graphs.size() || !h->graphs[(size_t)graph]) return fail(h, DVBS2HIP_EINVAL, "unknown graph");
    (void)hipGraphExecDestroy(h->graphs[(size_t)graph]);
    h->graphs[(size_t)graph] = nullptr;
    return 0;
}

int dvbs2hip_get_sizes(const dvbs2hip_t *h, dvbs2hip_sizes *o)
{
    if (!h || !o) return DVBS2HIP_EINVAL;
    o->N_ldpc = h->N_ldpc; o->K_ldpc = h->K_ldpc; o->K_bch = h->K_bch; o->bps = h->bps;
    o->N_xfec_sym = h->n_sym; o->pl_frame_sym = h->pl_frame; o->ldpc_edges = h->ldpc.E; o->ldpc_q = h->ldpc.q;
    return 0;
}

// ------------------------------------------------------------------ a1
// ch: ldpc_choice(h, F).  info_out / bch_flag only where ch.writes_info / ch.writes_bch
static int ldpc_dev(dvbs2hip_t *h, const LdpcChoice &ch, const float *Y, int8_t *CWD, int32_t *V, uint32_t *packed, float *post, int32_t *ites, int F, int32_t *info_out = nullptr,
                    uint8_t *bch_flag = nullptr, int8_t *cwd_bch = nullptr)
{
    if (!ch.error.empty()) return fail(h, DVBS2HIP_EUNSUPPORTED, ch.error);
    LdpcKParams p;
    memset(&p, 0, sizeof p);
    p.llr = Y; p.bits = V; p.packed = packed; p.cwd = CWD; p.post = post; p.ites = ites; p.gwork = h->d_gwork;
    p.info_out = info_out; p.info_prbs = h->bch.d_prbs_rw; p.K_info = h->K_bch;
    if (info_out && bch_flag) { p.syn_tab = h->d_syn_pos; p.info_prbs_s = h->d_prbs_s; p.syn_words = h->syn_words; p.syn_rows = h->syn_rows; p.bch_flag = bch_flag; p.cwd_bch = cwd_bch; }
    p.n_frames = F; p.n_ite = h->n_ite; p.early_stop = h->early_stop; p.alpha = h->alpha;
    if (h->ldpc_sched == DVBS2HIP_SCHED_NATURAL) {
        LdpcPlan &pl = h->ldpc;
        if (!h->d_nat_work || !pl.d_nat_tab || !pl.d_nat_haz) {
            const size_t bytes = ((size_t)h->max_frames + 63) / 64 * ldpc_nat_group_words(pl) * sizeof(float);
            if (!h->d_nat_work && dev_alloc(h, &h->d_nat_work, bytes, "natural-order LDPC: workspace of " + std::to_string(bytes) + " bytes does not fit")) return DVBS2HIP_ENOMEM;
            // a failed upload leaves its pointer null (or is freed here), so the next call tries again instead of launching with null tables
            if (!pl.d_nat_tab && upload(h, &pl.d_nat_tab, pl.nat_tab)) { (void)dev_free(h, &pl.d_nat_tab); return DVBS2HIP_EHIP; }
            if (!pl.d_nat_haz && upload(h, &pl.d_nat_haz, pl.nat_haz)) { (void)dev_free(h, &pl.d_nat_haz); return DVBS2HIP_EHIP; }
        }
    }
    Timer tm(h, DVBS2HIP_K_LDPC);
    // (round 6, measured NEGATIVE and therefore opt-in: DVBS2HIP_LDPC_ORDER=1) with the stopping rule the work queue can hand out the noisiest frames first
    // (frame_order_launch).  Same-box A/B of the reference's configuration, 2 M frames per point: 8.30 / 13.33 / 18.05 Gb/s at 3.6 / 3.7 / 3.8 dB in index order against
    // 8.16 / 13.09 / 17.98 ordered (three clones: 22.5 -> 21.3 at 3.8 dB; QPSK-N: -4 %): the queue already balances the workgroups, the frames that run to the cap are not
    // what a launch waits for -- the two small kernels and the lost locality cost more than the order gives (docs/negative_results.md, round 6).
    if (ch.takes_order) {
        void *dord;
        int r = ensure(h, B_ORDER, (size_t)F * 8, &dord);
        if (r) return r;
        HIPCHK(h, frame_order_launch(Y, (float *)dord + F, (uint32_t *)dord, F, h->N_ldpc, h->stream));
        p.order = (const uint32_t *)dord;
    }
    HIPCHK(h, ldpc_launch(h->ldpc, ch, p, h->d_nat_work, h->stream));
    return 0;
}

int dvbs2hip_ldpc_decode_siho_dev(dvbs2hip_t *h, const float *Y_N, int8_t *CWD, int32_t *V_K, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!Y_N || !V_K) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    return ldpc_dev(h, ldpc_choice(h, F), Y_N, CWD, V_K, nullptr, nullptr, nullptr, F);
}

int dvbs2hip_ldpc_decode_siho_post(dvbs2hip_t *h, const float *Y_N, int8_t *CWD, int32_t *V_K, float *post, int32_t *ites, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    const size_t nin = (size_t)F * h->N_ldpc * 4;
    std::vector<HostSock> outs = {{V_K, B_OUT, (size_t)F * h->K_ldpc * 4}, {CWD, B_CWD0, (size_t)F, 0, true}};
    if (post) outs.push_back({post, B_AUX0, nin});          // (asked for or not staged at all: the decoder takes null for "not wanted")
    if (ites) outs.push_back({ites, B_AUX1, (size_t)F * 4});
    return host_call(h, F, !post && !ites, {{Y_N, B_IN, nin}}, outs, [&](void *const *i, void *const *o, int nf) {
        return ldpc_dev(h, ldpc_choice(h, nf), (const float *)i[0], (int8_t *)o[1], (int32_t *)o[0], nullptr, (float *)(post ? o[2] : nullptr), (int32_t *)(ites ? o[outs.size() - 1] : nullptr), nf);
    });
}

int dvbs2hip_ldpc_decode_siho(dvbs2hip_t *h, const float *Y_N, int8_t *CWD, int32_t *V_K, int32_t F)
{
    return dvbs2hip_ldpc_decode_siho_post(h, Y_N, CWD, V_K, nullptr, nullptr, F);
}

// ------------------------------------------------------------------ a2
static int bch_dev(dvbs2hip_t *h, const int32_t *Y, const uint32_t *packed, int8_t *CWD, int32_t *V, bool descramble, int F, bool patch_only = false, const uint8_t *flag = nullptr)
{
    BchKParams p;
    memset(&p, 0, sizeof p);
    p.in_bits = Y; p.in_packed = packed; p.out_bits = V; p.cwd = CWD; p.n_frames = F; p.patch_only = patch_only ? 1 : 0; p.flag = flag;
    p.prbs = descramble ? h->bch.d_prbs : nullptr;
    Timer tm(h, DVBS2HIP_K_BCH);
    HIPCHK(h, bch_launch(h->bch, p, bch_grid(), h->stream));
    return 0;
}

int dvbs2hip_bch_decode_hiho_dev(dvbs2hip_t *h, const int32_t *Y_N, int8_t *CWD, int32_t *V_K, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!Y_N || !V_K) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    return bch_dev(h, Y_N, nullptr, CWD, V_K, false, F);
}

int dvbs2hip_bch_decode_hiho(dvbs2hip_t *h, const int32_t *Y_N, int8_t *CWD, int32_t *V_K, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    return host_call(h, F, false, {{Y_N, B_IN, (size_t)F * h->K_ldpc * 4}}, {{V_K, B_OUT, (size_t)F * h->K_bch * 4}, {CWD, B_CWD0, (size_t)F, 0, true}},
                     [&](void *const *i, void *const *o, int nf) { return bch_dev(h, (const int32_t *)i[0], nullptr, (int8_t *)o[1], (int32_t *)o[0], false, nf); });
}

// ------------------------------------------------------------------ a3 / a4
static FrontKParams front_params(dvbs2hip_t *h, const float *in, const float *sigma, float *llr, float *est, int F)
{
    FrontKParams p;
    memset(&p, 0, sizeof p);
    p.in = in; p.sigma_in = sigma; p.llr = llr; p.est = est; p.cstl = h->d_cstl; p.pl_seq = h->d_pl_seq;
    p.n_sym = h->n_sym; p.pl_frame = h->pl_frame; p.bps = h->bps; p.itl_cols = h->itl_cols; p.itl_order = h->itl_order;
    p.n_frames = F; p.code_rate = h->code_rate;
    p.sep = h->sep; for (int b = 0; b < 2; b++) { p.sep_ax[b] = h->sep_ax[b]; p.sep_g[b] = h->sep_g[b]; p.sep_h[b] = h->sep_h[b]; }
    return p;
}

// the call's facts for front_choose (rx_dispatch.h): plain values, the sockets as their alignment
static FrontChoice front_choice(const FrontKParams &p, bool from_pl, bool deinterleave)
{
    return front_choose({p.bps, p.sep != 0, p.itl_cols, p.n_sym, p.pl_frame, p.n_frames, ptr_align(p.in), ptr_align(p.llr), p.src != nullptr, from_pl, deinterleave});
}

static int demod_any_dev(dvbs2hip_t *h, const float *CP, const float *Y1, float *Y2, bool deitl, int F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!CP || !Y1 || !Y2) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    Timer tm(h, DVBS2HIP_K_DEMAP);
    const FrontKParams fp = front_params(h, Y1, CP, Y2, nullptr, F);
    HIPCHK(h, front_launch(fp, front_choice(fp, false, deitl), h->stream));
    return 0;
}

static int demod_any_host(dvbs2hip_t *h, const float *CP, const float *Y1, float *Y2, bool deitl, int F)
{
    int r = check_frames(h, F); if (r) return r;
    return host_call(h, F, false, {{Y1, B_IN, (size_t)F * 2 * h->n_sym * 4}, {CP, B_SIG, (size_t)F * 4}}, {{Y2, B_OUT, (size_t)F * h->N_ldpc * 4}},
                     [&](void *const *i, void *const *o, int nf) { return demod_any_dev(h, (const float *)i[1], (const float *)i[0], (float *)o[0], deitl, nf); });
}

int dvbs2hip_demodulate_dev(dvbs2hip_t *h, const float *CP, const float *Y1, float *Y2, int32_t F) { return demod_any_dev(h, CP, Y1, Y2, false, F); }
int dvbs2hip_demodulate(dvbs2hip_t *h, const float *CP, const float *Y1, float *Y2, int32_t F) { return demod_any_host(h, CP, Y1, Y2, false, F); }
int dvbs2hip_demodulate_deinterleave_dev(dvbs2hip_t *h, const float *CP, const float *Y1, float *nat, int32_t F) { return demod_any_dev(h, CP, Y1, nat, true, F); }
int dvbs2hip_demodulate_deinterleave(dvbs2hip_t *h, const float *CP, const float *Y1, float *nat, int32_t F) { return demod_any_host(h, CP, Y1, nat, true, F); }

int dvbs2hip_deinterleave_dev(dvbs2hip_t *h, const float *itl, float *nat, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!itl || !nat) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, deinterleave_launch(itl, nat, h->N_ldpc, h->itl_cols, h->itl_order, F, h->stream));
    return 0;
}

int dvbs2hip_host_register(dvbs2hip_t *h, void *ptr, size_t bytes)
{
    if (!h || !ptr || !bytes) return DVBS2HIP_EINVAL;
    if (hipSetDevice(h->device) != hipSuccess) return fail(h, DVBS2HIP_EHIP, "hipSetDevice failed");
    if (host_is_pinned(h, ptr, bytes)) return 0;
    hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) return fail(h, DVBS2HIP_EHIP, std::string("hipHostRegister: ") + hipGetErrorString(e));
    h->pinned[reinterpret_cast<uintptr_t>(ptr)] = bytes;
    return 0;
}

int dvbs2hip_host_unregister(dvbs2hip_t *h, void *ptr)
{
    if (!h || !ptr) return DVBS2HIP_EINVAL;
    auto it = h->pinned.find(reinterpret_cast<uintptr_t>(ptr));
    if (it == h->pinned.end()) return fail(h, DVBS2HIP_EINVAL, "this address was not registered");
    if (hipSetDevice(h->device) != hipSuccess) return fail(h, DVBS2HIP_EHIP, "hipSetDevice failed");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    (void)hipHostUnregister(ptr);
    h->pinned.erase(it);
    return 0;
}

int dvbs2hip_deinterleave(dvbs2hip_t *h, const float *itl, float *nat, int32_t F)
{
    return host_wrap<true>(h, itl, h ? h->N_ldpc : 0, nat, h ? h->N_ldpc : 0, F,
                           [&](const float *a, float *b, int nf) { return dvbs2hip_deinterleave_dev(h, a, b, nf); });
}

// ------------------------------------------------------------------ a6
int dvbs2hip_estimate_dev(dvbs2hip_t *h, const float *X, float *SIG, float *EB, float *ES, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!X || !SIG || !EB || !ES) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, estimate_launch(X, SIG, EB, ES, h->n_sym, h->code_rate, h->bps, F, h->stream));
    return 0;
}

int dvbs2hip_estimate(dvbs2hip_t *h, const float *X, float *SIG, float *EB, float *ES, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    const size_t nf4 = (size_t)F * 4;
    return host_call(h, F, false, {{X, B_IN, (size_t)F * 2 * h->n_sym * 4}}, {{SIG, B_OUT, nf4}, {EB, B_OUT, nf4, nf4}, {ES, B_OUT, nf4, 2 * nf4}},
                     [&](void *const *i, void *const *o, int nf) { return dvbs2hip_estimate_dev(h, (const float *)i[0], (float *)o[0], (float *)o[1], (float *)o[2], nf); });
}

// ------------------------------------------------------------------ a7
int dvbs2hip_pl_descramble_dev(dvbs2hip_t *h, const float *a, float *b, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!a || !b) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, pl_descramble_launch(a, b, h->d_pl_seq, h->pl_frame, F, h->stream));
    return 0;
}
int dvbs2hip_pl_descramble(dvbs2hip_t *h, const float *a, float *b, int32_t F)
{
    const size_t n = h ? (size_t)2 * h->pl_frame : 0;
    return host_wrap<true>(h, a, n, b, n, F, [&](const float *x, float *y, int nf) { return dvbs2hip_pl_descramble_dev(h, x, y, nf); });
}
int dvbs2hip_remove_plh_dev(dvbs2hip_t *h, const float *a, float *b, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!a || !b) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, remove_plh_launch(a, b, h->n_sym, h->pl_frame, F, h->stream));
    return 0;
}
int dvbs2hip_remove_plh(dvbs2hip_t *h, const float *a, float *b, int32_t F)
{
    return host_wrap<true>(h, a, h ? (size_t)2 * h->pl_frame : 0, b, h ? (size_t)2 * h->n_sym : 0, F,
                           [&](const float *x, float *y, int nf) { return dvbs2hip_remove_plh_dev(h, x, y, nf); });
}

// ------------------------------------------------------------------ a8
int dvbs2hip_bb_descramble_dev(dvbs2hip_t *h, const int32_t *a, int32_t *b, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!a || !b) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, bb_descramble_launch(a, b, h->bch.d_prbs, h->K_bch, F, h->stream));
    return 0;
}
int dvbs2hip_bb_descramble(dvbs2hip_t *h, const int32_t *a, int32_t *b, int32_t F)
{
    const size_t n = h ? (size_t)h->K_bch : 0;
    return host_wrap<true>(h, a, n, b, n, F, [&](const int32_t *x, int32_t *y, int nf) { return dvbs2hip_bb_descramble_dev(h, x, y, nf); });
}

// ------------------------------------------------------------------ fused RX baseband chain
// the chain's front end (PL descramble -> remove_plh -> estimate -> demodulate -> deinterleave in one launch): frame f read at pl + f 2 pl_frame, or where src[f] points;
// LLRs in natural order into llr, (sigma, Eb/N0, Es/N0) per frame into est
static int front_rx_dev(dvbs2hip_t *h, const float *pl, const float *const *src, const float *sigma, float *llr, float *est, int F)
{
    Timer tm(h, DVBS2HIP_K_FRONT);
    FrontKParams fp = front_params(h, pl, sigma, llr, est, F);
    fp.src = src;
    HIPCHK(h, front_launch(fp, front_choice(fp, true, true), h->stream));
    return 0;
}

static int rx_bb_any_dev(dvbs2hip_t *h, const float *pl, const float *const *src, const float *sigma, int32_t *info, int8_t *cwd_l, int8_t *cwd_b, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if ((!pl && !src) || !info) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    void *dllr, *dpk, *dest;
    const size_t nwords = (size_t)(h->K_ldpc + 31) / 32;
    if ((r = ensure(h, B_LLR, (size_t)F * h->N_ldpc * 4, &dllr)) || (r = ensure(h, B_PACKED, (size_t)F * nwords * 4, &dpk)) ||
        (r = ensure(h, B_EST, (size_t)F * 12, &dest)))
        return r;
    if ((r = front_rx_dev(h, pl, src, sigma, (float *)dllr, (float *)dest, F))) return r;
    // the LDPC kernel writes the descrambled info bits of every frame straight into the output socket (what the BCH stage outputs for a
    // frame it does not correct: nearly all of them behind a converged LDPC decoder); the BCH stage then only checks the syndromes of the
    // packed hard decisions and flips the bits it corrects -- its 4 K_bch output bytes per frame were 90 % of its time
    const LdpcChoice ch = ldpc_choice(h, F);
    const bool fused_out = ch.writes_info;
    // (round 5) ... and forms the frame's BCH remainder r(x) mod g(x) from the hard decisions it outputs: a frame whose remainder is zero is finished (information bits and
    // both CWD flags written by the LDPC kernel); the BCH stage rebuilds and decodes the flagged frames only
    void *dflag = nullptr;
    if (ch.writes_bch && (r = ensure(h, B_BCHFLAG, (size_t)F, &dflag))) return r;
    if ((r = ldpc_dev(h, ch, (const float *)dllr, cwd_l, nullptr, (uint32_t *)dpk, nullptr, nullptr, F, fused_out ? info : nullptr, (uint8_t *)dflag, cwd_b))) return r;
    return bch_dev(h, nullptr, (const uint32_t *)dpk, cwd_b, info, true, F, fused_out, (const uint8_t *)dflag);
}

int dvbs2hip_rx_bb_dev(dvbs2hip_t *h, const float *pl, const float *sigma, int32_t *info, int8_t *cwd_l, int8_t *cwd_b, int32_t F)
{
    if (h && !pl) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    return rx_bb_any_dev(h, pl, nullptr, sigma, info, cwd_l, cwd_b, F);
}

// (round 5) the fused chain behind dvbs2hip_sync_frame_locate_dev: frame f is read where SRC[f] points (device table of device pointers)
int dvbs2hip_rx_bb_located_dev(dvbs2hip_t *h, const float *const *SRC, const float *sigma, int32_t *info, int8_t *cwd_l, int8_t *cwd_b, int32_t F)
{
    if (h && !SRC) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if (h && h->bw.S > 1) return fail(h, DVBS2HIP_EUNSUPPORTED, "the located form is one stream per handle: with dvbs2hip_set_streams(S > 1) use dvbs2hip_rx_bb_dev on the synchronizer's Y_N2");
    return rx_bb_any_dev(h, nullptr, SRC, sigma, info, cwd_l, cwd_b, F);
}

int dvbs2hip_rx_bb(dvbs2hip_t *h, const float *pl, const float *sigma, int32_t *info, int8_t *cwd_l, int8_t *cwd_b, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    // sigma is optional and small: it goes up whole, ahead of the frames, also when these go through the pipeline
    return host_call(h, F, true, {{sigma, B_SIG, (size_t)F * 4, 0, true, true}, {pl, B_IN, (size_t)F * 2 * h->pl_frame * 4}},
                     {{info, B_INFO, (size_t)F * h->K_bch * 4}, {cwd_l, B_CWD0, (size_t)F, 0, true}, {cwd_b, B_CWD1, (size_t)F, 0, true}},
                     [&](void *const *i, void *const *o, int nf) { return dvbs2hip_rx_bb_dev(h, (const float *)i[1], (const float *)i[0], (int32_t *)o[0], (int8_t *)o[1], (int8_t *)o[2], nf); });
}

// ------------------------------------------------------------------ the fused chain's front end alone: what rx_bb hands its LDPC decoder, in the caller's sockets
int dvbs2hip_rx_front_dev(dvbs2hip_t *h, const float *pl, const float *sigma, float *LLR, float *EST, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!pl || !LLR || !EST) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    return front_rx_dev(h, pl, nullptr, sigma, LLR, EST, F);
}

int dvbs2hip_rx_front_located_dev(dvbs2hip_t *h, const float *const *SRC, const float *sigma, float *LLR, float *EST, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!SRC || !LLR || !EST) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    if (h->bw.S > 1) return fail(h, DVBS2HIP_EUNSUPPORTED, "the located form is one stream per handle: with dvbs2hip_set_streams(S > 1) use dvbs2hip_rx_front_dev on the synchronizer's Y_N2");
    return front_rx_dev(h, nullptr, SRC, sigma, LLR, EST, F);
}

int dvbs2hip_rx_front(dvbs2hip_t *h, const float *pl, const float *sigma, float *LLR, float *EST, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    return host_call(h, F, false, {{sigma, B_SIG, (size_t)F * 4, 0, true, true}, {pl, B_IN, (size_t)F * 2 * h->pl_frame * 4}},
                     {{LLR, B_LLR, (size_t)F * h->N_ldpc * 4}, {EST, B_EST, (size_t)F * 12}},
                     [&](void *const *i, void *const *o, int nf) { return dvbs2hip_rx_front_dev(h, (const float *)i[1], (const float *)i[0], (float *)o[0], (float *)o[1], nf); });
}

// ------------------------------------------------------------------ N1: TX mirror + AWGN
int dvbs2hip_tx_bb_dev(dvbs2hip_t *h, const int32_t *info_in, uint64_t seed, const float *sigma, int32_t *info_out, float *pl, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!pl) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    void *dbch, *dldpc;
    if ((r = ensure(h, B_TXBCH, (size_t)F * ((h->K_ldpc + 31) / 32) * 4, &dbch)) ||
        (r = ensure(h, B_TXLDPC, (size_t)F * ((h->N_ldpc + 31) / 32) * 4, &dldpc)))
        return r;
    TxKParams p;
    memset(&p, 0, sizeof p);
    p.info_in = info_in; p.info_out = info_out; p.sigma = sigma; p.pl_out = pl;
    p.bch_cw = (uint32_t *)dbch; p.ldpc_cw = (uint32_t *)dldpc; p.prbs = h->bch.d_prbs;
    p.enc_tab = h->d_enc_tab; p.enc_deg = h->d_enc_deg; p.cstl = h->d_cstl; p.plh = h->d_plh; p.pl_seq = h->d_pl_seq;
    p.bch_tab = h->d_bch_tab; p.bch_shift = h->d_bch_shift;
    p.seed_lo = (uint32_t)seed; p.seed_hi = (uint32_t)(seed >> 32);
    p.K_bch = h->K_bch; p.K_ldpc = h->K_ldpc; p.N_ldpc = h->N_ldpc; p.bps = h->bps; p.itl_cols = h->itl_cols; p.itl_order = h->itl_order;
    p.n_sym = h->n_sym; p.pl_frame = h->pl_frame; p.enc_stride = h->enc_stride; p.n_frames = F;
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, tx_launch(p, h->stream));
    return 0;
}

int dvbs2hip_tx_bb(dvbs2hip_t *h, const int32_t *info_in, uint64_t seed, const float *sigma, int32_t *info_out, float *pl, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    const size_t nb = (size_t)F * h->K_bch * 4;
    return host_call(h, F, false, {{info_in, B_IN, nb, 0, true}, {sigma, B_SIG, (size_t)F * 4, 0, true}}, {{info_out, B_INFO, nb, 0, true}, {pl, B_OUT, (size_t)F * 2 * h->pl_frame * 4}},
                     [&](void *const *i, void *const *o, int nf) { return dvbs2hip_tx_bb_dev(h, (const int32_t *)i[0], seed, (const float *)i[1], (int32_t *)o[0], (float *)o[1], nf); });
}

// ------------------------------------------------------------------ measurement + memory helpers
int dvbs2hip_timing_enable(dvbs2hip_t *h, int32_t on)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (h->capturing) return fail(h, DVBS2HIP_EINVAL, "a capture is open on this handle");
    h->timing = on != 0;
    return 0;
}
int dvbs2hip_timing_reset(dvbs2hip_t *h)
{
    if (!h) return DVBS2HIP_EINVAL;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < DVBS2HIP_K_COUNT; k++) {
        for (auto &p : h->ev[k]) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
        h->ev[k].clear();
    }
    return 0;
}
int dvbs2hip_timing_get(dvbs2hip_t *h, int32_t k, double *total_ms, int64_t *n)
{
    if (!h || k < 0 || k >= DVBS2HIP_K_COUNT || !total_ms || !n) return DVBS2HIP_EINVAL;
    int r0 = enter(h); if (r0) return r0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double tot = 0.0;
    for (auto &p : h->ev[k]) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, p.first, p.second));
        tot += ms;
    }
    *total_ms = tot; *n = (int64_t)h->ev[k].size();
    return 0;
}
// a plain streaming copy, 16 bytes per lane and access, U accesses in flight per lane; NT: non-temporal loads and stores.  Flat grid: workgroup b copies the
// U consecutive 4 KB pieces starting at piece b U (what the front end and the synchronizers' rotation do with their streams).
typedef float copy_f4 __attribute__((ext_vector_type(4)));
extern "C++" {
template <int U, bool NT>
__global__ void __launch_bounds__(256) device_copy_kernel(const copy_f4 *__restrict__ src, copy_f4 *__restrict__ dst, size_t n4)
{
    const size_t i0 = (size_t)blockIdx.x * (256 * U) + threadIdx.x;
    copy_f4 v[U];
#pragma unroll
    for (int k = 0; k < U; k++) { const size_t i = i0 + (size_t)k * 256; if (i < n4) v[k] = NT ? __builtin_nontemporal_load(&src[i]) : src[i]; }
#pragma unroll
    for (int k = 0; k < U; k++) { const size_t i = i0 + (size_t)k * 256; if (i < n4) { if (NT) __builtin_nontemporal_store(v[k], &dst[i]); else dst[i] = v[k]; } }
}
}  // extern "C++"

int dvbs2hip_device_copy_bandwidth(dvbs2hip_t *h, size_t bytes, int32_t reps, double *GBps)
{
    if (!h || !GBps || reps < 1 || bytes < 16) return DVBS2HIP_EINVAL;
    int r0 = enter(h); if (r0) return r0;
    const size_t n4 = bytes / 16;
    void *a = nullptr, *b = nullptr;
    if (hipMalloc(&a, n4 * 16) != hipSuccess) return fail(h, DVBS2HIP_ENOMEM, "hipMalloc of " + std::to_string(n4 * 16) + " bytes failed");
    if (hipMalloc(&b, n4 * 16) != hipSuccess) { (void)hipFree(a); return fail(h, DVBS2HIP_ENOMEM, "hipMalloc of " + std::to_string(n4 * 16) + " bytes failed"); }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    double best = 0.0;
    if (hipMemsetAsync(a, 0x3c, n4 * 16, h->stream) != hipSuccess || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = DVBS2HIP_EHIP;
    // the best of four shapes (1 / 4 accesses in flight per lane, plain / non-temporal): which one wins depends on the size against the Infinity Cache
    for (int shape = 0; shape < 4 && !rc; shape++) {
        const int U = shape & 1 ? 4 : 1;
        const unsigned grid = (unsigned)((n4 + (size_t)256 * U - 1) / ((size_t)256 * U));
        auto launch = [&]() {
            if (shape == 0) hipLaunchKernelGGL((device_copy_kernel<1, false>), dim3(grid), dim3(256), 0, h->stream, (const copy_f4 *)a, (copy_f4 *)b, n4);
            else if (shape == 1) hipLaunchKernelGGL((device_copy_kernel<4, false>), dim3(grid), dim3(256), 0, h->stream, (const copy_f4 *)a, (copy_f4 *)b, n4);
            else if (shape == 2) hipLaunchKernelGGL((device_copy_kernel<1, true>), dim3(grid), dim3(256), 0, h->stream, (const copy_f4 *)a, (copy_f4 *)b, n4);
            else hipLaunchKernelGGL((device_copy_kernel<4, true>), dim3(grid), dim3(256), 0, h->stream, (const copy_f4 *)a, (copy_f4 *)b, n4);
        };
        float ms = 0.f;
        launch();      // warm-up
        (void)hipEventRecord(e0, h->stream);
        for (int i = 0; i < reps; i++) launch();
        (void)hipEventRecord(e1, h->stream);
        if (hipStreamSynchronize(h->stream) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) rc = DVBS2HIP_EHIP;
        else { const double g = 2.0 * (double)(n4 * 16) * reps / ((double)ms * 1e-3) / 1e9; if (g > best) best = g; }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(a); (void)hipFree(b);
    if (rc) return fail(h, rc, "device copy measurement failed");
    *GBps = best;
    return 0;
}

int dvbs2hip_malloc(dvbs2hip_t *h, void **d, size_t bytes)
{
    if (!h || !d) return DVBS2HIP_EINVAL;
    int r0 = enter(h); if (r0) return r0;
    if (hipMalloc(d, bytes) != hipSuccess) return fail(h, DVBS2HIP_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
    return 0;
}
int dvbs2hip_free(dvbs2hip_t *h, void *d) { int r0 = enter(h); if (r0) return r0; HIPCHK(h, hipFree(d)); return 0; }
int dvbs2hip_memcpy_h2d(dvbs2hip_t *h, void *dst, const void *src, size_t bytes)
{
    int r0 = enter(h); if (r0) return r0;
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}
int dvbs2hip_memcpy_d2h(dvbs2hip_t *h, void *dst, const void *src, size_t bytes)
{
    int r0 = enter(h); if (r0) return r0;
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
