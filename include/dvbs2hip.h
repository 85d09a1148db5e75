/*
 * dvbs2hip.h -- C ABI of libdvbs2hip.so: the DVB-S2 RX inner path on AMD MI355X (gfx950).
 *
 * Drop-in boundary: each entry point replaces the body of ONE task codelet
 * of the reference (aff3ct/dvbs2).  The "replaces" lines cite the reference interface
 * (path:line relative to /root/reference).  Sockets of the reference hold n_frames
 * frames contiguously (frame f at offset f * n_elmts); so do all buffers here.
 *
 * Conventions
 *   - plain C, opaque handle, no exceptions across the ABI
 *   - return value: 0 = success, < 0 = dvbs2hip_status error (text: dvbs2hip_last_error)
 *   - B = int32_t (one bit per int, 0/1), R = Q = float, as in the reference (H6)
 *   - entry points WITHOUT suffix take HOST pointers (socket semantics): H2D copy,
 *     kernels, D2H copy, stream synchronised on return
 *   - entry points WITH `_dev` take DEVICE pointers, enqueue on the handle's stream and
 *     return without synchronising (chained tasks avoid PCIe round trips)
 *   - 1 <= n_frames <= cfg.max_frames; inter-frame batching (-F) maps to the grid width
 *   - a handle is entered by one host thread at a time (a StreamPU module instance is
 *     only ever entered by one thread: SURVEY.md 8b "Threading")
 *   - there is NO CPU fallback: without a usable HIP device dvbs2hip_create fails
 */
#ifndef DVBS2HIP_H
#define DVBS2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVBS2HIP_VERSION 101

typedef enum {
    DVBS2HIP_OK           = 0,
    DVBS2HIP_EINVAL       = -1,  /* spu::tools::invalid_argument / length_error        */
    DVBS2HIP_ENOMEM       = -2,  /* spu::tools::cannot_allocate                        */
    DVBS2HIP_EHIP         = -3,  /* spu::tools::runtime_error (HIP runtime failure)    */
    DVBS2HIP_EUNSUPPORTED = -4,  /* spu::tools::unimplemented_error                    */
    DVBS2HIP_ENODEVICE    = -5,  /* no HIP device: the product never falls back to CPU */
    DVBS2HIP_ETIMEOUT     = -6   /* dvbs2hip_monitor_reduce: a peer rank did not arrive within the timeout given at _reduce_init (it died): the communicator is
                                    aborted, the handle's stream is no longer usable -- the caller should leave with a non-zero exit code (a fresh exit, no re-exec) */
} dvbs2hip_status;

typedef struct dvbs2hip_handle dvbs2hip_t;

/* LDPC check-node rule (--dec-implem, DVBS2.cpp:117-149; the reference's default is SPA) */
enum { DVBS2HIP_IMPLEM_NMS = 0, DVBS2HIP_IMPLEM_MS = 1,
       DVBS2HIP_IMPLEM_SPA = 2,          /* sum-product as the reference decodes it: the exact check node with every message clipped at 2 atanh(1 - FLT_EPSILON) = 16.64, where
                                            the messages of AFF3CT's Update_rule_SPA saturate (fp32 tanh product) -- frame for frame the decisions of SPA_TANH on 99.9 % of the
                                            frames near the waterfall (results/r06/spa_rules.md); within 1e-4 max(1, |L|) of the oracle's ORC_SPA_CLIP */
       DVBS2HIP_IMPLEM_SPA_TANH = 3,   /* sum-product as AFF3CT's Update_rule_SPA evaluates it [UPSTREAM-RECALL]: tanh product in fp32, messages capped at
                                            2 atanh(1 - FLT_EPSILON) = 16.64; BIT-EXACT against the oracle's ORC_SPA_TANH (every operation correctly rounded) */
       DVBS2HIP_IMPLEM_SPA_EXACT = 4 };  /* the exact check node without the clip (rounds 1-5's SPA): within 1e-4 max(1, |L|) of the oracle's ORC_SPA; loses 20-50 % more frames than the
                                            reference at the low-FER end of the rate-3/5 traces and has an error floor below them (results/r06/spa_rules.md) */
/* Order in which the layered decoder visits the checks of a frame (dvbs2hip_set_ldpc_schedule) */
enum { DVBS2HIP_SCHED_QC = 0,        /* quasi-cyclic layers of 360 independent checks: the throughput path */
       DVBS2HIP_SCHED_NATURAL = 1 }; /* natural row order of H, what AFF3CT's BP_HORIZONTAL_LAYERED runs: one lane per frame */
/* Interleaver read order (DVBS2.cpp:300-317) */
enum { DVBS2HIP_ITL_TOP_LEFT = 0, DVBS2HIP_ITL_TOP_RIGHT = 1 };

/*
 * Configuration = the arguments the reference passes to its build_* functions
 * (DVBS2.cpp:287-356 modcod_init, :406-495 builders).  Pointers are only read during
 * dvbs2hip_create.  dvbs2hip_cfg_from_modcod fills everything for a named MODCOD.
 */
typedef struct dvbs2hip_cfg {
    /* code sizes */
    int32_t N_ldpc;            /* 16200 | 64800                                   */
    int32_t K_ldpc;            /* = N_bch                                         */
    int32_t K_bch;
    /* LDPC: ETSI EN 302 307 Annex B/C address table, K_ldpc/360 rows              */
    int32_t        ldpc_n_rows;
    const int32_t *ldpc_row_ptr;   /* n_rows + 1                                  */
    const int32_t *ldpc_addr;
    int32_t ldpc_n_ite;        /* --dec-ite                                       */
    int32_t ldpc_implem;       /* DVBS2HIP_IMPLEM_*                               */
    float   ldpc_alpha;        /* NMS normalisation factor; 1.0 = AFF3CT default  */
    int32_t ldpc_early_stop;   /* 1: stop on zero syndrome (enable_syndrome)      */
    /* BCH: GF(2^m) primitive polynomial (coefficient of x^i at [i], m+1 entries), t */
    int32_t        bch_m;
    int32_t        bch_t;
    const int32_t *bch_prim;
    /* modem: raw constellation (2^bps points, re/im interleaved, conf/mod order);  */
    /* normalised to unit mean energy inside, like tools::Constellation_user        */
    int32_t      bps;
    const float *cstl;
    /* bit interleaver: itl_cols <= 1 means Interleaver_core_NO                     */
    int32_t itl_cols;
    int32_t itl_order;
    /* matched filter: real taps (as Filter_RRC_ccr_naive::compute_rrc_coefs returns */
    /* them); fir_n_taps = 0 disables the filter entry points                       */
    int32_t      fir_n_taps;
    const float *fir_taps;
    int32_t      fir_osf;      /* samples per symbol of the filter input           */
    /* runtime */
    int32_t max_frames;        /* capacity of one call (the -F of the socket), 1 .. 65534.  A handle for at most one frame per CU (<= 256) decodes N = 64800 with the
                                  one-frame-per-CU kernel: lower latency per call (0.42 against 0.54 ms), same results bit for bit */
    int32_t device;            /* HIP device ordinal                               */
    void   *stream;            /* hipStream_t to enqueue on, or NULL: own stream   */
    int32_t ldpc_lds_groups;   /* tuning: < 0 = automatic                          */
    /* PLS code of the PLHEADER: the 7-entry mod_cod vector of Framer.hxx:111-126 (TX side only) */
    int32_t pls[7];
} dvbs2hip_cfg;

/* ------------------------------------------------------------------ lifecycle */
/* Names accepted: the reference's five ("QPSK-S_8/9", "QPSK-S_3/5", "8PSK-S_3/5",
 * "8PSK-S_8/9", "16APSK-S_8/9"; "" = "QPSK-S_8/9": DVBS2.cpp:287-319) plus the extension
 * rows "QPSK-N_8/9", "8PSK-N_8/9", "16APSK-N_8/9", "32APSK-S_3/4".  Unknown name:
 * DVBS2HIP_EINVAL (the reference throws invalid_argument, DVBS2.cpp:319).  Fills code
 * sizes, tables, constellation, interleaver and the 81-tap SRRC (Shaping_filter.hpp:24-28);
 * implem = SPA, n_ite = 50, alpha = 1, early_stop = 1, max_frames = 1 (the reference's defaults,
 * DVBS2.cpp:135-142). */
int dvbs2hip_cfg_from_modcod(const char *modcod, dvbs2hip_cfg *cfg);
int dvbs2hip_create(const dvbs2hip_cfg *cfg, dvbs2hip_t **out);
/* GPUs this process sees (0 without one): what a one-process-per-GPU launcher takes `cfg.device = local_rank % count` from when the
 * environment gives it a global rank only (host/dvbs2_tx_rx_bb.cpp); the reference's analogue is the thread count of Sequence(first, n_threads),
 * TX_RX_BB/main.cpp:96. */
int dvbs2hip_device_count(int32_t *count);
void dvbs2hip_destroy(dvbs2hip_t *h);
/* text of the last error on this handle (or of the last failed create when h == NULL) */
const char *dvbs2hip_last_error(const dvbs2hip_t *h);
/* selects the check order of ldpc_decode_siho / rx_bb on this handle (default DVBS2HIP_SCHED_QC).  NATURAL reproduces the
 * reference's horizontal-layered sweep (checks 0 .. M-1 in row order) exactly as the oracle's ORC_SCHED_NATURAL does; it
 * keeps 4 (N + 3 M) bytes of state per frame in HBM (22 MB per 64 normal frames, allocated on first use for max_frames)
 * and only pays off on batches of tens of thousands of frames.  NMS / MS only: DVBS2HIP_EUNSUPPORTED otherwise. */
int dvbs2hip_set_ldpc_schedule(dvbs2hip_t *h, int32_t schedule);
/* name of the LDPC kernel instantiation the plan selected for this MODCOD (diagnostics, bench.py's roofline line) */
const char *dvbs2hip_ldpc_kernel_name(const dvbs2hip_t *h);
/* Pins a host socket buffer (hipHostRegister) for the lifetime of the handle or until _unregister.  With every socket of a
 * call pinned, dvbs2hip_ldpc_decode_siho and dvbs2hip_rx_bb copy at PCIe speed and run the batch in chunks with the two copy
 * directions and the kernels overlapped (host-form QPSK normal frames: 29 k -> ~150 k frames/s); unpinned sockets keep the plain
 * copy -> kernels -> copy path.  StreamPU socket buffers live as long as their module, so an integration registers each once
 * after binding.  The buffer must stay allocated while registered. */
int dvbs2hip_host_register(dvbs2hip_t *h, void *ptr, size_t bytes);
int dvbs2hip_host_unregister(dvbs2hip_t *h, void *ptr);
/* Interface_reset: clears the filter state and the monitor counters */
int dvbs2hip_reset(dvbs2hip_t *h);
/* change --dec-ite / alpha / early-stop without rebuilding tables */
int dvbs2hip_set_ldpc_params(dvbs2hip_t *h, int32_t n_ite, float alpha, int32_t early_stop);
void *dvbs2hip_get_stream(dvbs2hip_t *h);      /* hipStream_t */
int dvbs2hip_synchronize(dvbs2hip_t *h);
/* A sequence of _dev calls as ONE submission (hipGraph; BASELINE configs[4], small-frame latency: at -F 1 the sequence filter -> extract -> rx_bb is six launches and a fill
 * around one workgroup's ten iterations).  Between _begin and _end the _dev calls of this handle are RECORDED, not run (same pointers, same n_frames on every replay; no host-
 * socket form, no dvbs2hip_synchronize in between; _begin returns DVBS2HIP_EINVAL while dvbs2hip_timing_enable is on; run the sequence once before recording it: first calls allocate).  Tasks that keep a memory from call to call (filter, shape_filter, the synchronizers) are recorded with the memory buffers of that moment: every replay starts from the state the stream had when the
 * sequence was recorded, which is what a latency measurement on one frame wants and NOT a way to run a stream; dvbs2hip_sync_coarse_synchronize_dev, whose stream position is a launch argument, refuses to be recorded.  The reference's counterpart is the task
 * sequence itself (RX/main_sched.cpp:199-223: a spu::runtime::Sequence runs its bound tasks back to back). */
int dvbs2hip_graph_begin(dvbs2hip_t *h);
int dvbs2hip_graph_end(dvbs2hip_t *h, int32_t *graph);
int dvbs2hip_graph_launch(dvbs2hip_t *h, int32_t graph);
int dvbs2hip_graph_destroy(dvbs2hip_t *h, int32_t graph);
/* derived sizes (per frame), as DVBS2.cpp:351-355 */
typedef struct dvbs2hip_sizes {
    int32_t N_ldpc, K_ldpc, K_bch, bps, N_xfec_sym, pl_frame_sym, ldpc_edges, ldpc_q;
} dvbs2hip_sizes;
int dvbs2hip_get_sizes(const dvbs2hip_t *h, dvbs2hip_sizes *out);

/* ------------------------------------------------------------------ a1  LDPC decoder
 * replaces: module::Decoder_SIHO::decode_siho(Y_N, CWD, V_K) of the decoder returned by
 * tools::Codec_LDPC<B,Q>::get_decoder_siho() -- built DVBS2.cpp:418-449, bound
 * TX_RX_BB/main.cpp:65,90-91 (sockets dec::sck::decode_siho::{Y_N,CWD,V_K}).
 *   Y_N : float  [n_frames * N_ldpc]  channel LLRs, LLR > 0 <=> bit 0
 *   CWD : int8_t [n_frames]           1 = codeword detected (zero syndrome)
 *   V_K : int32_t[n_frames * K_ldpc]  hard decisions of the systematic bits        */
int dvbs2hip_ldpc_decode_siho(dvbs2hip_t *h, const float *Y_N, int8_t *CWD, int32_t *V_K, int32_t n_frames);
int dvbs2hip_ldpc_decode_siho_dev(dvbs2hip_t *h, const float *Y_N, int8_t *CWD, int32_t *V_K, int32_t n_frames);
/* test hook: also returns the N_ldpc posteriors (natural order) and the iteration count */
int dvbs2hip_ldpc_decode_siho_post(dvbs2hip_t *h, const float *Y_N, int8_t *CWD, int32_t *V_K,
                                   float *post_N, int32_t *n_ite_done, int32_t n_frames);

/* ------------------------------------------------------------------ a2  BCH decoder
 * replaces: Decoder_BCH_DVBS2<B,R>::_decode_hiho(const B *Y_N, int8_t *CWD, B *V_K, frame_id)
 * -- src/common/Module/Decoder_BCH_DVBS2/Decoder_BCH_DVBS2.cpp:28-40 (bit reversal around
 * Decoder_BCH_std::_decode), built DVBS2.cpp:406-416, bound TX_RX_BB/main.cpp:91-92.
 *   Y_N : int32_t[n_frames * K_ldpc]   V_K : int32_t[n_frames * K_bch]   CWD = !status */
int dvbs2hip_bch_decode_hiho(dvbs2hip_t *h, const int32_t *Y_N, int8_t *CWD, int32_t *V_K, int32_t n_frames);
int dvbs2hip_bch_decode_hiho_dev(dvbs2hip_t *h, const int32_t *Y_N, int8_t *CWD, int32_t *V_K, int32_t n_frames);

/* ------------------------------------------------------------------ a3  soft demapper
 * replaces: module::Modem_generic_fast<B,R,Q,max_star>::demodulate(CP, Y_N1, Y_N2)
 * -- built DVBS2.cpp:478-488, bound TX_RX_BB/main.cpp:87-88.
 *   CP  : float[n_frames]              sigma (per real dimension), one per frame
 *   Y_N1: float[n_frames * 2*N_xfec]   symbols, re/im interleaved
 *   Y_N2: float[n_frames * N_ldpc]     LLRs in transmission (interleaved) order      */
int dvbs2hip_demodulate(dvbs2hip_t *h, const float *CP, const float *Y_N1, float *Y_N2, int32_t n_frames);
int dvbs2hip_demodulate_dev(dvbs2hip_t *h, const float *CP, const float *Y_N1, float *Y_N2, int32_t n_frames);

/* ------------------------------------------------------------------ a4  LLR de-interleaver
 * replaces: module::Interleaver<float,uint32_t>::deinterleave(itl, nat)
 * -- DVBS2.cpp:451-476, bound TX_RX_BB/main.cpp:56,89.                              */
int dvbs2hip_deinterleave(dvbs2hip_t *h, const float *itl, float *nat, int32_t n_frames);
int dvbs2hip_deinterleave_dev(dvbs2hip_t *h, const float *itl, float *nat, int32_t n_frames);
/* a3+a4 fused (one pass, permuted store) */
int dvbs2hip_demodulate_deinterleave(dvbs2hip_t *h, const float *CP, const float *Y_N1, float *nat, int32_t n_frames);
int dvbs2hip_demodulate_deinterleave_dev(dvbs2hip_t *h, const float *CP, const float *Y_N1, float *nat, int32_t n_frames);

/* ------------------------------------------------------------------ a5  SRRC matched filter
 * replaces: Filter<R>::filter(X_N1, Y_N2) -> Filter_FIR_ccr<R>::_filter
 * -- src/common/Module/Filter/Filter_FIR/Filter_FIR_ccr.cpp:68-142 (+ step(),
 * Filter_FIR_ccr.hpp:39-52), bound RX/main_sched.cpp:199-201.  The n_frames frames of
 * one call are consecutive in time; the last (n_taps-1) complex samples are kept in the
 * handle between calls (Filter_FIR_ccr.cpp:80-83); dvbs2hip_filter_reset zeroes them.
 * After dvbs2hip_set_streams(h, S > 1) the call carries S streams (stream s = frames
 * [s F/S, (s+1) F/S), n_frames a multiple of S), each with a memory of its own, and stream s
 * is filtered exactly as a one-stream call on its frames alone; dvbs2hip_filter_reset zeroes
 * every stream's memory.  filter / filter1 follow it; filter2 has no memory and does not.
 *   X_N1, Y_N2 : float[n_frames * 2 * n_cplx]                                        */
int dvbs2hip_filter(dvbs2hip_t *h, const float *X_N1, float *Y_N2, int32_t n_cplx, int32_t n_frames);
int dvbs2hip_filter_dev(dvbs2hip_t *h, const float *X_N1, float *Y_N2, int32_t n_cplx, int32_t n_frames);
int dvbs2hip_filter_reset(dvbs2hip_t *h);
/* replaces: Filter<R>::filter1(X_N1, Y_N2) and ::filter2(X_N1, Y_N2h, Y_N2) -> Filter_FIR_ccr<R>::_filter1 / _filter2
 * -- Filter_FIR_ccr.cpp:144-218 and :220-294; tasks and sockets flt::tsk::{filter1,filter2}, flt::sck::filter1::{X_N1,Y_N2},
 * flt::sck::filter2::{X_N1,Y_N2h,Y_N2} (Filter.hpp:22-29, codelets Filter.hxx:69-96); bound RX/main_sched.cpp:199-201 and split
 * over two pipeline stages in main_13-sta.cpp:274-282.  The reference's filter1 writes the outputs below about half a frame and
 * advances the filter state; its filter2 copies Y_N2h and computes the rest from X_N1 alone.  Same here, as pure functions of
 * the sockets (the two tasks may run in different pipeline stages on different batches):
 *   filter1: Y_N2[f][0 .. split) = the filtered frame, state advanced exactly as dvbs2hip_filter does.  (The samples from
 *            `split` on, which the reference leaves as they were, are filled as well -- nothing may depend on them.)
 *   filter2: Y_N2[f][0 .. split) = Y_N2h[f][0 .. split);  Y_N2[f][split .. n_cplx) computed from X_N1[f] only; no state read
 *            or written.  filter2(X, filter1(X)) == filter(X) bit for bit.
 * split = dvbs2hip_filter_split(h, n_cplx) complex samples (n_cplx / 2 rounded down to a multiple of 4; the reference's own
 * split depends on its SIMD width).  Half a frame has to hold the filter's memory: n_cplx / 2 >= n_taps - 1, else EINVAL
 * (the reference reads out of bounds in that case).   X_N1, Y_N2h, Y_N2 : float[n_frames * 2 * n_cplx]                  */
int dvbs2hip_filter_split(const dvbs2hip_t *h, int32_t n_cplx);
int dvbs2hip_filter1(dvbs2hip_t *h, const float *X_N1, float *Y_N2, int32_t n_cplx, int32_t n_frames);
int dvbs2hip_filter1_dev(dvbs2hip_t *h, const float *X_N1, float *Y_N2, int32_t n_cplx, int32_t n_frames);
int dvbs2hip_filter2(dvbs2hip_t *h, const float *X_N1, const float *Y_N2h, float *Y_N2, int32_t n_cplx, int32_t n_frames);
int dvbs2hip_filter2_dev(dvbs2hip_t *h, const float *X_N1, const float *Y_N2h, float *Y_N2, int32_t n_cplx, int32_t n_frames);
/* Kernel behind dvbs2hip_filter[_dev] on this handle.  AUTO (default): the matrix-core form (bf16 x 3 split operands,
 * fp32 accumulation, k_fir_mfma.hip) for filters of at most 81 taps on 16-byte aligned sockets, the fp32 vector kernel
 * otherwise; VALU forces the vector kernel; MFMA returns DVBS2HIP_EUNSUPPORTED for a longer filter.  Both meet the same
 * 1e-4 bar against Filter_FIR_ccr's fp32 FMA chain (neither reproduces its rounding order bit for bit). */
enum { DVBS2HIP_FIR_AUTO = 0, DVBS2HIP_FIR_VALU = 1, DVBS2HIP_FIR_MFMA = 2 };
int dvbs2hip_set_filter_kernel(dvbs2hip_t *h, int32_t kernel);

/* ------------------------------------------------------------------ a6  noise estimator
 * replaces: Estimator<R>::estimate(X_N, SIG, Eb_N0, Es_N0) -> Estimator_DVBS2<R>::_estimate
 * -- src/common/Module/Estimator/Estimator_DVBS2.hxx:31-58, wrapper Estimator.hxx:103-118.
 *   X_N : float[n_frames * 2*N_xfec]; SIG, Eb_N0, Es_N0 : float[n_frames]            */
int dvbs2hip_estimate(dvbs2hip_t *h, const float *X_N, float *SIG, float *Eb_N0, float *Es_N0, int32_t n_frames);
int dvbs2hip_estimate_dev(dvbs2hip_t *h, const float *X_N, float *SIG, float *Eb_N0, float *Es_N0, int32_t n_frames);

/* ------------------------------------------------------------------ the gain stages of the RX graph
 * replaces: Multiplier_AGC_cc_naive::imultiply -> _imultiply
 * -- src/common/Module/Multiplier/Sequence/Multiplier_AGC_cc_naive.cpp:22-46 (task / sockets Multiplier.hxx:49-60): every frame is divided by its standard deviation
 * about its mean over sqrt(output_energy).  The reference builds two: `front_agc` on the received samples (n_cplx = pl_frame * osf, output_energy = 1 / osf: DVBS2.cpp:660-664,
 * bound RX/main_sched.cpp:197-198) and `mult_agc` on the symbols behind the timing synchronizer, in front of the frame synchronizer (n_cplx = pl_frame, output_energy = 1:
 * DVBS2.cpp:653-657, bound RX/main_sched.cpp:205-207).  A frame of equal values divides by zero as it does there.
 *   X_N: float[n_frames * 2*n_cplx]  ->  Z_N: same size                                                   */
int dvbs2hip_agc_imultiply(dvbs2hip_t *h, const float *X_N, float *Z_N, int32_t n_cplx, float output_energy, int32_t n_frames);
int dvbs2hip_agc_imultiply_dev(dvbs2hip_t *h, const float *X_N, float *Z_N, int32_t n_cplx, float output_energy, int32_t n_frames);

/* The coarse frequency synchronizer's task in the TRANSMISSION phase: the frequency shift alone
 * replaces: Synchronizer_freq_coarse::synchronize -> Synchronizer_freq_coarse_DVBS2_aib::_synchronize = Multiplier_sine_ccc_naive::imultiply
 * -- src/common/Module/Synchronizer/Synchronizer_freq/Synchronizer_freq_coarse/Synchronizer_freq_coarse_DVBS2_aib.cpp:43-50, Multiplier/Sine/Multiplier_sine_ccc_naive.cpp:69-77
 * (sockets X_N1 / FRQ / PHS / Y_N2: Synchronizer_freq_coarse.hxx:35-39; bound RX/main_sched.cpp:198-200).  z_n = x_n exp(j omega n), n the position in the stream (it starts
 * over after 999999; the frequency is kept to six decimals so that this is seamless).  The LOOP that finds the frequency (update_phase, :53-95, one step per pilot symbol fed back
 * from the timing synchronizer) is sample-serial and out of scope: _set_freq takes what it, or anything else, has estimated.  FRQ / PHS per frame: that frequency and 0.
 *   X_N1: float[n_frames * 2*n_cplx] -> Y_N2: same size (frames = consecutive stretches of ONE stream)             */
int dvbs2hip_sync_coarse_set_freq(dvbs2hip_t *h, float estimated_freq);
int dvbs2hip_sync_coarse_reset(dvbs2hip_t *h);
int dvbs2hip_sync_coarse_synchronize(dvbs2hip_t *h, const float *X_N1, float *FRQ, float *PHS, float *Y_N2, int32_t n_cplx, int32_t n_frames);
int dvbs2hip_sync_coarse_synchronize_dev(dvbs2hip_t *h, const float *X_N1, float *FRQ, float *PHS, float *Y_N2, int32_t n_cplx, int32_t n_frames);

/* ------------------------------------------------------------------ a7  PL descramble, header/pilot removal
 * replaces: Scrambler_PL<D>::descramble -> __scramble(scr_flag = false)
 * -- src/common/Module/Scrambler/Scrambler_PL/Scrambler_PL.hxx:61-78 (start_ix = 90)
 *   Y_N1, Y_N2 : float[n_frames * 2*pl_frame]                                        */
int dvbs2hip_pl_descramble(dvbs2hip_t *h, const float *Y_N1, float *Y_N2, int32_t n_frames);
int dvbs2hip_pl_descramble_dev(dvbs2hip_t *h, const float *Y_N1, float *Y_N2, int32_t n_frames);
/* replaces: Framer<B>::remove_plh -> _remove_plh -- src/common/Module/Framer/Framer.hxx:330-343
 *   Y_N1 : float[n_frames * 2*pl_frame] -> Y_N2 : float[n_frames * 2*N_xfec]         */
int dvbs2hip_remove_plh(dvbs2hip_t *h, const float *Y_N1, float *Y_N2, int32_t n_frames);
int dvbs2hip_remove_plh_dev(dvbs2hip_t *h, const float *Y_N1, float *Y_N2, int32_t n_frames);

/* ------------------------------------------------------------------ a8  BB descramble
 * replaces: Scrambler_BB<D>::_descramble -- src/common/Module/Scrambler/Scrambler_BB/Scrambler_BB.hxx:51-72
 *   Y_N1, Y_N2 : int32_t[n_frames * K_bch]                                           */
int dvbs2hip_bb_descramble(dvbs2hip_t *h, const int32_t *Y_N1, int32_t *Y_N2, int32_t n_frames);
int dvbs2hip_bb_descramble_dev(dvbs2hip_t *h, const int32_t *Y_N1, int32_t *Y_N2, int32_t n_frames);

/* ------------------------------------------------------------------ a9  BER/FER monitor
 * replaces: module::Monitor_BFER<B>::check_errors(U, V) -- built DVBS2.cpp:575-591, bound
 * TX_RX_BB/main.cpp:93-94.  Counters {FRA, BE, FE} live on the device; get copies them out
 * (what tools::Monitor_reduction sums across threads, main.cpp:123-125, is summed across
 * GPUs by the host with one 24-byte all-reduce: DESIGN.md "multi-GPU").
 *   U, V : int32_t[n_frames * K_bch]                                                 */
int dvbs2hip_monitor_check_errors(dvbs2hip_t *h, const int32_t *U, const int32_t *V, int32_t n_frames);
int dvbs2hip_monitor_check_errors_dev(dvbs2hip_t *h, const int32_t *U, const int32_t *V, int32_t n_frames);
int dvbs2hip_monitor_get(dvbs2hip_t *h, uint64_t fra_be_fe[3]);
int dvbs2hip_monitor_reset(dvbs2hip_t *h);
/* replaces: module::Monitor_BFER<B>::check_errors2(U, V, FRA, BE, FE, BER, FER) -- the task the RX mains bind
 * (RX/main_sched.cpp:222-223 U / V, :244-247 BE / FE / BER / FER into probes; aff3ct, absent: sockets
 * mnt::sck::check_errors2::{U,V,FRA,BE,FE,BER,FER}).  Counts like check_errors AND writes the monitor's counters as they
 * stand after each frame of the call (frame f of the socket = state after frames 0..f): FRA int64, BE / FE int32,
 * BER = BE / FRA / K_bch and FER = FE / FRA as float, with Monitor_BFER's convention that before the first bit error they
 * report the bound 1 / FRA [/ K_bch] instead of 0.  Any of the five output pointers may be NULL.
 *   U, V : int32_t[n_frames * K_bch];  FRA : int64_t[n_frames];  BE, FE : int32_t[n_frames];  BER, FER : float[n_frames]   */
int dvbs2hip_monitor_check_errors2(dvbs2hip_t *h, const int32_t *U, const int32_t *V, int64_t *FRA, int32_t *BE, int32_t *FE,
                                   float *BER, float *FER, int32_t n_frames);
int dvbs2hip_monitor_check_errors2_dev(dvbs2hip_t *h, const int32_t *U, const int32_t *V, int64_t *FRA, int32_t *BE, int32_t *FE,
                                       float *BER, float *FER, int32_t n_frames);
/* replaces: tools::Monitor_reduction over the per-thread monitors (TX_RX_BB/main.cpp:123-125 construction + 500 ms period,
 * :155-161 is_done_all / final reduction) for ONE PROCESS PER GPU: the sum of {FRA, BE, FE} over the ranks, one RCCL
 * all-reduce of 3 x uint64 on the handle's stream (over xGMI inside a node).  COLLECTIVE: every rank calls _reduce the same
 * number of times (call it once per batch, as is_done_all is).  librccl.so is opened at run time on the first _init.
 *   init    : rank 0 creates the communicator id and hands it to the other ranks through files named after `rendezvous_path`
 *             (dvbs2hip_rendezvous below); each side waits for at most timeout_ms (< 0: for ever).  world_size 1 needs no file.
 *             ncclCommInitRank itself has no timeout: a launcher has to end the whole job when one rank dies.
 *   reduce  : the reduced counters; on a handle without _init it is dvbs2hip_monitor_get (a single process).  With timeout_ms > 0 at _init a reduction whose peers do
 *             not arrive within timeout_ms returns DVBS2HIP_ETIMEOUT (the communicator is aborted; leave with a non-zero exit code) instead of waiting for ever.
 *   finalize: destroys the communicator (also done by dvbs2hip_destroy).                                              */
int dvbs2hip_monitor_reduce_init(dvbs2hip_t *h, int32_t rank, int32_t world_size, const char *rendezvous_path, int32_t timeout_ms);
/* the out-of-band step of _reduce_init on its own (no GPU needed): rank 0 hands `bytes` bytes of `blob` to every other rank, which
 * receives them in `blob`.  Files left by an earlier run are harmless: rank r publishes a fresh random nonce in `<path>.hello.<r>` and takes
 * the payload only from a `<path>.ack.<r>` that repeats it; a completed exchange leaves no file behind.  Give every job a path of its own
 * in a directory only its user can write.  0, DVBS2HIP_EINVAL (bad arguments, cannot write) or DVBS2HIP_EHIP (timed out).                */
int dvbs2hip_rendezvous(int32_t rank, int32_t world_size, const char *rendezvous_path, void *blob, size_t bytes, int32_t timeout_ms);
int dvbs2hip_monitor_reduce(dvbs2hip_t *h, uint64_t fra_be_fe[3]);
int dvbs2hip_monitor_reduce_finalize(dvbs2hip_t *h);

/* ------------------------------------------------------------------ fused RX baseband chain (a7 -> a8)
 * One call = the RX half of TX_RX_BB/main.cpp:83-92:
 *   PL descramble -> remove_plh -> estimate -> demodulate -> deinterleave -> LDPC
 *   decode_siho -> BCH decode_hiho -> BB descramble, all intermediates device-resident.
 *   pl_frames: float  [n_frames * 2*pl_frame]
 *   sigma_in : float  [n_frames] or NULL (NULL: Estimator_DVBS2; else Estimator_perfect)
 *   info_bits: int32_t[n_frames * K_bch]
 *   cwd_ldpc, cwd_bch: int8_t[n_frames] (either may be NULL)                         */
int dvbs2hip_rx_bb(dvbs2hip_t *h, const float *pl_frames, const float *sigma_in, int32_t *info_bits,
                   int8_t *cwd_ldpc, int8_t *cwd_bch, int32_t n_frames);
int dvbs2hip_rx_bb_dev(dvbs2hip_t *h, const float *pl_frames, const float *sigma_in, int32_t *info_bits,
                       int8_t *cwd_ldpc, int8_t *cwd_bch, int32_t n_frames);
/* the fused chain reading frame f where SRC[f] points (the table dvbs2hip_sync_frame_locate_dev fills): same outputs as dvbs2hip_rx_bb_dev on the delayed copy */
int dvbs2hip_rx_bb_located_dev(dvbs2hip_t *h, const float *const *SRC, const float *sigma, int32_t *info_bits, int8_t *cwd_ldpc, int8_t *cwd_bch, int32_t n_frames);

/* ------------------------------------------------------------------ the fused chain's front end alone (a7 -> a6 -> a3 -> a4)
 * The first launch of dvbs2hip_rx_bb* with its two outputs in the caller's sockets instead of the handle's private buffers: what the chain's LDPC decoder is handed.
 *   pl_frames: float[n_frames * 2*pl_frame]      SRC: as dvbs2hip_rx_bb_located_dev (DVBS2HIP_EUNSUPPORTED while dvbs2hip_set_streams(S > 1), likewise)
 *   sigma_in : float[n_frames] or NULL (NULL: the M2M4 estimate of the frame's own payload symbols)
 *   LLR      : float[n_frames * N_ldpc], natural (code) order: the input of dvbs2hip_ldpc_decode_siho
 *   EST      : float[n_frames * 3] = (sigma, Eb/N0 dB, Es/N0 dB) per frame; with sigma_in given (sigma_in[f], 0, 0)
 * Same code path as the chain (one helper launches both), and the kernels write straight into LLR / EST.  Which kernel form runs depends on the sockets as it does inside
 * the chain: the QPSK pair form needs pl_frames and LLR 16-byte aligned (the located form: LLR only) and takes the one-symbol form otherwise; the handle's own LLR buffer
 * is 256-byte aligned, so a 16-byte aligned LLR socket selects what dvbs2hip_rx_bb* selects for the same input.  The host form stages through device buffers of the handle. */
int dvbs2hip_rx_front(dvbs2hip_t *h, const float *pl_frames, const float *sigma_in, float *LLR, float *EST, int32_t n_frames);
int dvbs2hip_rx_front_dev(dvbs2hip_t *h, const float *pl_frames, const float *sigma_in, float *LLR, float *EST, int32_t n_frames);
int dvbs2hip_rx_front_located_dev(dvbs2hip_t *h, const float *const *SRC, const float *sigma, float *LLR, float *EST, int32_t n_frames);

/* ------------------------------------------------------------------ N1: TX mirror + AWGN channel (test-signal side)
 * One call = the TX half + channel of TX_RX_BB/main.cpp:75-82 on the device:
 *   Source::generate -> Scrambler_BB::scramble -> Encoder_BCH_DVBS2::encode
 *   (src/common/Module/Encoder_BCH_DVBS2/Encoder_BCH_DVBS2.cpp:28-43) -> LDPC encode (DVBS2.cpp:427)
 *   -> Interleaver::interleave -> Modem::modulate -> Framer::generate (Framer.hxx:232-293)
 *   -> Scrambler_PL::scramble (Scrambler_PL.hxx:61-78) -> Channel_AWGN::add_noise (DVBS2.cpp:593-613).
 *   info_in  : int32_t[n_frames * K_bch] or NULL (NULL: Source_random, Philox keyed by seed)
 *   sigma    : float[n_frames] noise std-dev per real dimension, or NULL for no noise
 *   info_out : int32_t[n_frames * K_bch] the payload that was sent (the monitor's U socket), or NULL
 *   pl_frames: float[n_frames * 2*pl_frame]                                             */
int dvbs2hip_tx_bb(dvbs2hip_t *h, const int32_t *info_in, uint64_t seed, const float *sigma, int32_t *info_out,
                   float *pl_frames, int32_t n_frames);
int dvbs2hip_tx_bb_dev(dvbs2hip_t *h, const int32_t *info_in, uint64_t seed, const float *sigma, int32_t *info_out,
                       float *pl_frames, int32_t n_frames);

/* ------------------------------------------------------------------ TX tasks: one entry per codelet of the transmitter
 * The seven tasks the reference's TX mains bind between the source and the shaping filter (src/mains/TX/main.cpp:70-78,
 * TX_VAR/main.cpp:71-78, TX_RX_BB/main.cpp:75-81), sockets as there: one int32_t per bit (0 or 1; other input values are
 * not defined, outputs are exactly 0 or 1), re/im interleaved floats per symbol.  Input and output sockets are distinct; the
 * tasks keep no state between calls.  Chained in this order they compute what dvbs2hip_tx_bb computes without noise.
 * _dev sockets may start at any multiple of the element size (4 bytes for bits, 8 for a complex symbol).
 *
 * replaces: Scrambler_BB<B>::scramble -> _scramble -- src/common/Module/Scrambler/Scrambler_BB/Scrambler_BB.hxx:51-72
 * (the same XOR as dvbs2hip_bb_descramble).
 *   X_N1, X_N2 : int32_t[n_frames * K_bch]                                            */
int dvbs2hip_bb_scramble(dvbs2hip_t *h, const int32_t *X_N1, int32_t *X_N2, int32_t n_frames);
int dvbs2hip_bb_scramble_dev(dvbs2hip_t *h, const int32_t *X_N1, int32_t *X_N2, int32_t n_frames);
/* replaces: Encoder_BCH_DVBS2<B>::encode -> _encode -- src/common/Module/Encoder_BCH_DVBS2/Encoder_BCH_DVBS2.cpp:28-43.
 * Systematic: X_N[0 .. K_bch) = U_K, then the N_bch - K_bch parity bits, coefficient of the highest power first.
 *   U_K : int32_t[n_frames * K_bch]  ->  X_N : int32_t[n_frames * N_bch]   (N_bch = K_ldpc)       */
int dvbs2hip_bch_encode(dvbs2hip_t *h, const int32_t *U_K, int32_t *X_N, int32_t n_frames);
int dvbs2hip_bch_encode_dev(dvbs2hip_t *h, const int32_t *U_K, int32_t *X_N, int32_t n_frames);
/* replaces: the LDPC encoder's encode (enc type "LDPC_DVBS2", built src/common/Factory/DVBS2/DVBS2.cpp:427; ETSI EN 302 307
 * 5.3.2).  Systematic: X_N[0 .. K_ldpc) = U_K, then the parity bits p_0 .. p_{M-1} in natural order.
 *   U_K : int32_t[n_frames * K_ldpc]  ->  X_N : int32_t[n_frames * N_ldpc]                       */
int dvbs2hip_ldpc_encode(dvbs2hip_t *h, const int32_t *U_K, int32_t *X_N, int32_t n_frames);
int dvbs2hip_ldpc_encode_dev(dvbs2hip_t *h, const int32_t *U_K, int32_t *X_N, int32_t n_frames);
/* replaces: module::Interleaver<B,uint32_t>::interleave(nat, itl) -- the column/row interleaver of DVBS2.cpp:451-476:
 * itl[i] = nat[lut[i]]; a copy when the MODCOD has none (itl_cols == 1).
 *   nat, itl : int32_t[n_frames * N_ldpc]                                             */
int dvbs2hip_interleave(dvbs2hip_t *h, const int32_t *nat, int32_t *itl, int32_t n_frames);
int dvbs2hip_interleave_dev(dvbs2hip_t *h, const int32_t *nat, int32_t *itl, int32_t n_frames);
/* replaces: module::Modem_generic<B,R,Q>::modulate(X_N1, X_N2) -- built DVBS2.cpp:478-488.  Symbol k takes bits
 * k bps .. k bps + bps - 1, bit b with weight 1 << b, and is the handle's normalised constellation point of that index.
 *   X_N1 : int32_t[n_frames * N_ldpc]  ->  X_N2 : float[n_frames * 2*N_xfec]          */
int dvbs2hip_modulate(dvbs2hip_t *h, const int32_t *X_N1, float *X_N2, int32_t n_frames);
int dvbs2hip_modulate_dev(dvbs2hip_t *h, const int32_t *X_N1, float *X_N2, int32_t n_frames);
/* replaces: Framer<B>::generate -> _generate -- src/common/Module/Framer/Framer.hxx:232-293: the 90 PLHEADER symbols, then the
 * data with a block of 36 pilots after every 16 slots.
 *   Y_N1 : float[n_frames * 2*N_xfec]  ->  Y_N2 : float[n_frames * 2*pl_frame]        */
int dvbs2hip_framer_generate(dvbs2hip_t *h, const float *Y_N1, float *Y_N2, int32_t n_frames);
int dvbs2hip_framer_generate_dev(dvbs2hip_t *h, const float *Y_N1, float *Y_N2, int32_t n_frames);
/* replaces: Scrambler_PL<D>::scramble -> __scramble(scr_flag = true)
 * -- src/common/Module/Scrambler/Scrambler_PL/Scrambler_PL.hxx:46,61-78 (start_ix = 90): the header is copied, symbol
 * i >= 90 is turned by R[i - 90] quarter turns (swaps and sign changes: no rounding).
 *   X_N1, X_N2 : float[n_frames * 2*pl_frame]                                         */
int dvbs2hip_pl_scramble(dvbs2hip_t *h, const float *X_N1, float *X_N2, int32_t n_frames);
int dvbs2hip_pl_scramble_dev(dvbs2hip_t *h, const float *X_N1, float *X_N2, int32_t n_frames);

/* ------------------------------------------------------------------ N2: TX shaping filter, channel noise, perfect timing
 * replaces: Filter_UPRRC_ccr_naive::filter -> Filter_UPFIR_ccr_naive::_filter
 * -- src/common/Module/Filter/Filter_UPFIR/Filter_UPFIR_ccr_naive.cpp:52-66 (polyphase bank of `fir_osf` FIRs built
 * from the handle's taps), bound src/mains/TX_RX/main.cpp:212,223.  Keeps (n_taps-1)/osf input samples between calls.
 *   X_N1: float[n_frames * 2*n_cplx]  ->  Y_N2: float[n_frames * 2*n_cplx*osf]                    */
int dvbs2hip_shape_filter(dvbs2hip_t *h, const float *X_N1, float *Y_N2, int32_t n_cplx, int32_t n_frames);
int dvbs2hip_shape_filter_dev(dvbs2hip_t *h, const float *X_N1, float *Y_N2, int32_t n_cplx, int32_t n_frames);
/* replaces: Channel_AWGN::add_noise(CP, X_N, Y_N) -- built DVBS2.cpp:593-613, bound TX_RX_BB/main.cpp:81-82.
 *   CP: float[n_frames] sigma per real value; X_N, Y_N: float[n_frames * n_elmts] (n_elmts even)   */
int dvbs2hip_add_noise(dvbs2hip_t *h, const float *CP, const float *X_N, float *Y_N, uint64_t seed, int32_t n_elmts, int32_t n_frames);
int dvbs2hip_add_noise_dev(dvbs2hip_t *h, const float *CP, const float *X_N, float *Y_N, uint64_t seed, int32_t n_elmts, int32_t n_frames);
/* perfect-timing extraction (Synchronizer_timing_perfect, DVBS2.cpp:558-570): the batch is ONE stream,
 * Y[i] = X[offset + i*osf] for i < n_frames*n_cplx_out; samples outside the batch read as zero.      */
int dvbs2hip_extract_dev(dvbs2hip_t *h, const float *X, float *Y, int32_t n_cplx_out, int32_t osf, int64_t offset, int32_t n_frames);

/* ------------------------------------------------------------------ symbol-timing recovery (the reference's `--stm-type FAST`)
 * replaces: Synchronizer_timing::synchronize -> Synchronizer_Gardner_fast_osf2::_synchronize and Synchronizer_timing::extract -> _extract
 * -- src/common/Module/Synchronizer/Synchronizer_timing/Synchronizer_Gardner_fast_osf2.cpp:35-198 (Farrow interpolator Filter_Farrow_ccr_naive.hxx, Gardner detector,
 * PI loop filter, NCO), Synchronizer_timing.hxx:48-78 (tasks and sockets), :189-201 (MU), :243-304 (extract: the carry buffer and the underflow count); built by
 * Factory/Module/Synchronizer_timing/Synchronizer_timing.cpp:91-96, bound RX/main_sched.cpp:202-204.  Frames of pl_frame * osf complex samples; osf = 2 only (the handle's
 * fir_osf; the NORMAL and osf != 2 variants are not provided: DVBS2HIP_EUNSUPPORTED; ULTRA is chosen with dvbs2hip_sync_timing_set_type, below).  Results are bit for bit the CPU twin's (tests/timing_twin.c), which restates the reference's order of operations.
 * Streams: the n_frames frames of a call are S streams of n_frames / S consecutive frames each, stream s = frames [s F/S, (s+1) F/S) (F a multiple of S, else EINVAL).
 * S = 1 (the default) is the reference's module: one stream.  Every stream keeps its own loop state and carry buffer in the handle between calls; one lane runs one stream.
 * F/S is fixed by the first call after a reset (or set_streams): a call with another F/S returns EINVAL until dvbs2hip_sync_timing_reset.
 *   synchronize: X_N1 float[F * 2 N] -> Y_N1 float[F * 2 N] (interpolated samples), B_N1 int32_t[F * 2 N] (1 on both reals of a strobe), MU float[F] (mu after the frame)
 *   extract    : Y_N1, B_N1 -> Y_N2 float[F * N] (N = pl_frame * osf reals = pl_frame symbols per frame), UFW int32_t[F], RDY int32_t[S]
 * extract fills a stream's frames with the reals its carry buffer held, then the strobed reals of Y_N1; what does not fit stays in the carry buffer (at most 4 N F/S reals,
 * four calls' worth of output: a stream whose strobes run that far ahead of its output loses the excess and reports RDY[s] = 2 -- the reference grows its buffer instead).  A stream with too few reals (the reference throws processing_aborted) is NOT READY: RDY[s] = 0, all it had stays
 * in the carry buffer for the next call, its frames of Y_N2 hold only the reals it had (the rest of the socket is left as it was) and the frame they reached counts an underflow.
 * UFW[f] = the underflows counted on frame slot f since the stream's last ready call, this call's included; a ready call reports them and clears them.
 * set_params: damping factor, normalized bandwidth, detector gain (defaults sqrt(0.5), 5e-5, 2: Synchronizer_timing.hpp:28-30); get_gains returns the loop filter's proportional
 * and integrator gains (set_loop_filter_coeffs, .cpp:188-198).  set_streams and reset clear every stream's state, carry buffer and underflow counts.
 * Graph capture: these tasks keep a memory, so the rule of dvbs2hip_graph_begin holds -- a replay starts from the state recorded; set_streams / reset refuse an open capture. */
int dvbs2hip_sync_timing_set_params(dvbs2hip_t *h, float damping, float nbw, float detector_gain);
int dvbs2hip_sync_timing_get_gains(dvbs2hip_t *h, float *proportional, float *integrator);
int dvbs2hip_sync_timing_set_streams(dvbs2hip_t *h, int32_t S);
/* S independent streams per call in every receive task that keeps a memory: stream s = frames [s F/S, (s+1) F/S) of a call.
 * = dvbs2hip_sync_timing_set_streams(h, S) (timing, step_mf, coarse shift: as above) AND the block-wise matched filter (dvbs2hip_filter / filter1), the frame synchronizer
 * (synchronize1 / synchronize2 / synchronize) and L&R (dvbs2hip_sync_lr_synchronize), which dvbs2hip_sync_timing_set_streams alone leaves at one stream: the handle keeps
 * two counts, this entry sets both.  The default is 1, and a handle that never calls it behaves in every entry as it did before the entry existed.  S < 1 or S > max_frames
 * (or > 65535): DVBS2HIP_EINVAL; an open capture: DVBS2HIP_EINVAL.  It clears every stream's state of all the tasks it governs, also when S does not change (S = 1: the
 * resets of the timing tasks, the matched filter, the frame synchronizer -- with the SOF delay, the previous output frame and the last metric, as a new handle -- and L&R).
 * In the three block-wise tasks n_frames must be a multiple of S (else DVBS2HIP_EINVAL); unlike the timing tasks F/S may change from call to call.  Per stream the
 * operations are those of a one-stream handle fed that stream's frames in the same calls: same results, bit for bit (L&R: those of its three-kernel form, DVBS2HIP_LR=unfused).
 * Per-stream state is allocated by the first call that needs it (inside a capture: run the sequence once before); a failed allocation returns DVBS2HIP_ENOMEM and leaves
 * the handle with the state it had.  dvbs2hip_sync_frame_get_metric writes S entries per output; dvbs2hip_sync_frame_reset, dvbs2hip_sync_lr_reset and
 * dvbs2hip_filter_reset clear all streams.  With S > 1 L&R always runs as three kernels (pilots, one workgroup per stream for the recurrence, rotation): no workgroup
 * waits for another, and dvbs2hip_sync_lr_timeouts keeps counting one-launch calls only.
 * What stays one stream per handle: the located form (dvbs2hip_sync_frame_locate_dev and dvbs2hip_rx_bb_located_dev return DVBS2HIP_EUNSUPPORTED while S > 1: "one run of
 * the input stream" is an argument about one stream), the task sequences above the C ABI (RxSequence, acquire) and the host/ modules, and the TX / channel side:
 * filter2 (no memory), shape_filter, channel_delay, channel_freq_shift, add_noise.  Every stateless receive task takes the frames of S streams in one call anyway. */
int dvbs2hip_set_streams(dvbs2hip_t *h, int32_t S);
int dvbs2hip_sync_timing_reset(dvbs2hip_t *h);
int dvbs2hip_sync_timing_synchronize(dvbs2hip_t *h, const float *X_N1, float *Y_N1, int32_t *B_N1, float *MU, int32_t n_frames);
int dvbs2hip_sync_timing_synchronize_dev(dvbs2hip_t *h, const float *X_N1, float *Y_N1, int32_t *B_N1, float *MU, int32_t n_frames);
int dvbs2hip_sync_timing_extract(dvbs2hip_t *h, const float *Y_N1, const int32_t *B_N1, float *Y_N2, int32_t *UFW, int32_t *RDY, int32_t n_frames);
int dvbs2hip_sync_timing_extract_dev(dvbs2hip_t *h, const float *Y_N1, const int32_t *B_N1, float *Y_N2, int32_t *UFW, int32_t *RDY, int32_t n_frames);
/* The held Gardner loop (the reference's `--stm-type ULTRA --stm-hold-size H`)
 * replaces: Synchronizer_Gardner_ultra_osf2::_synchronize -- Synchronizer_timing/Synchronizer_Gardner_ultra_osf2.cpp:59-133 (hold blocks, control samples, the tail),
 * .hxx:58-120 (TED_update, loop_filter, interpolation_control), :341-351 (the gains: FAST's formula); Synchronizer_timing::set_act, Synchronizer_timing.hxx:109 and
 * RX/main_sched.cpp:655; built by Factory/Module/Synchronizer_timing/Synchronizer_timing.cpp from --stm-type ULTRA, --stm-hold-size (default 101).
 * set_type chooses the loop behind dvbs2hip_sync_timing_synchronize / _dev: DVBS2HIP_STM_FAST (the default; hold_size is ignored) or DVBS2HIP_STM_ULTRA with its hold size
 * (hold_size <= 4 with ULTRA: DVBS2HIP_EINVAL, the reference's assertion).  It clears every stream's state like set_streams and refuses an open capture.  The sockets, the
 * streams rule and the F/S rule are those above; extract is the same task behind either loop.  A handle that never calls set_type is the FAST loop.
 * set_act: while it is clear (after create, set_type, reset: Synchronizer_timing::reset clears it) ULTRA runs the whole loop on every sample; once it is set -- the reference
 * sets it when its learning phases are over -- every frame is cut into N / hold_size blocks (N = pl_frame * osf; the blocks start over at every frame) that hold mu over
 * their first hold_size - 4 samples and run the whole loop on the last four, and a tail of N mod hold_size samples with the whole loop.  The flag is a launch argument: a
 * captured graph keeps the value it was recorded with.  It is stored for FAST too and has no effect there.
 * One wave runs one stream, its lanes across the held samples of a block (S streams are S waves).  Results are bit for bit the CPU twin's (tests/timing_ultra_twin.c).
 * In the _dev form X_N1 and Y_N1 must not overlap under ULTRA: the kernel reads a sample's three predecessors from X_N1 after it has written their outputs.
 * Not provided yet: ULTRA's detector inside the coarse-frequency loop.  While the type is ULTRA dvbs2hip_sync_step_mf_synchronize / _dev return DVBS2HIP_EUNSUPPORTED (the
 * loop's sample-by-sample `step` with ULTRA's forms of TED_update and loop_filter is a later change). */
enum { DVBS2HIP_STM_FAST = 0, DVBS2HIP_STM_ULTRA = 1 };
int dvbs2hip_sync_timing_set_type(dvbs2hip_t *h, int32_t type, int32_t hold_size);
int dvbs2hip_sync_timing_set_act(dvbs2hip_t *h, int32_t act);
/* The channel's three delay tasks, in the order CH/main.cpp:60-62 and TX_RX/main.cpp:215-218 bind them (test-signal side)
 * replaces: Filter_buffered_delay::filter ((floor(D) - 2) / N frames), Variable_delay_cc_naive::filter ((floor(D) - 2 + N) % N samples), Filter_Farrow_ccr_naive::filter
 * (mu = D - floor(D)) -- built DVBS2.cpp:520-544 from --chn-max-delay D >= 2 (DVBS2.cpp:128-133).  The two delay lines start at zero and compose to one of floor(D) - 2 samples;
 * the frames of a call are consecutive in one stream and the last floor(D) + 1 samples are kept in the handle between calls.  set_delay clears that memory.
 *   X, Y: float[n_frames * 2 N], N = pl_frame * osf complex samples.  Graph capture: as above (a task with a memory).                                   */
int dvbs2hip_channel_set_delay(dvbs2hip_t *h, float D);
int dvbs2hip_channel_delay(dvbs2hip_t *h, const float *X, float *Y, int32_t n_frames);
int dvbs2hip_channel_delay_dev(dvbs2hip_t *h, const float *X, float *Y, int32_t n_frames);

/* The channel's frequency shift, the task between the fractional delay and the noise (CH/main.cpp:63-64)
 * replaces: Multiplier_sine_ccc_naive::imultiply built by DVBS2.cpp:624-626 from --chn-max-freq-shift (cycles per sample, floored to six decimals; Fs = 1): the stream times
 * exp(j 2 pi nu n), n = 0 .. 999999 the stream position.  set_freq_shift starts the position over.  X, Y: float[n_frames * 2 N], N = pl_frame * osf.  Graph capture: refused,
 * as dvbs2hip_sync_coarse_synchronize_dev (the stream position is a launch argument). */
int dvbs2hip_channel_set_freq_shift(dvbs2hip_t *h, float freq_shift);
int dvbs2hip_channel_freq_shift(dvbs2hip_t *h, const float *X, float *Y, int32_t n_frames);
int dvbs2hip_channel_freq_shift_dev(dvbs2hip_t *h, const float *X, float *Y, int32_t n_frames);

/* ------------------------------------------------------------------ the coarse-frequency loop (the reference's waiting and learning phases 1-2, RX/main_sched.cpp:407-560)
 * replaces: Synchronizer_step_mf_cc::synchronize -- src/common/Module/Synchronizer/Synchronizer_step_mf_cc.cpp:163-208: per complex sample the coarse synchronizer's rotation
 * (Multiplier_sine_ccc_naive::step), the 81-tap matched filter's step (Filter_FIR_ccr_naive.hpp:36-49), the timing synchronizer's step (Synchronizer_Gardner_fast_osf2.hxx:8-87)
 * and, on a strobe, Synchronizer_freq_coarse_DVBS2_aib::update_phase (.cpp:57-92: the pilot-aided detector, PI filter, integrator, set_nu(-estimated_freq)); once per frame
 * curr_idx = (N_out - DEL + last_delay) mod (N_out / 2) from the frame synchronizer's delay of the call before (the reference's Feedbacker).
 *   DEL int32_t[F], X_N1 float[F * 2 N] -> MU, FRQ, PHS float[F] (mu, estimated_freq, 0 after each frame), Y_N1 float[F * 2 N], B_N1 int32_t[F * 2 N]; N = pl_frame * 2
 * Y_N1 / B_N1 are what dvbs2hip_sync_timing_extract takes.  Streams as for the timing entries (dvbs2hip_sync_timing_set_streams; one lane per stream).  Results are bit
 * for bit the CPU twin's (tests/stepmf_twin.c); its header states the two places where the arithmetic is this library's own: the rotation evaluates cos / sin of the exact
 * turn fraction (nu n mod 1) and the matched filter sums 41 symmetric products in a fixed order.
 * State is shared with the block-wise tasks, as the reference's modules share theirs: the loop runs on the timing synchronizer's per-stream state (so that
 * dvbs2hip_sync_timing_synchronize / _extract carry on from it), on the coarse synchronizer's frequency and sample counter (so that dvbs2hip_sync_coarse_synchronize carries
 * on with the learned frequency and a continuous phase; with S streams that state is per stream, and set_freq sets all of them) and, with one stream, on the matched
 * filter's memory (dvbs2hip_filter / filter1 carry on from it and back).  With S > 1 the same holds per stream when the block-wise filter runs on the same S streams
 * (dvbs2hip_set_streams: every stream's last 80 samples cross the switch between the loop and dvbs2hip_filter*, in both directions); after dvbs2hip_sync_timing_set_streams
 * alone the block-wise filter is one stream and the loop keeps a memory per stream of its own.
 * set_pll = set_PLL_coeffs(pll_sps, damping, nbw) (.cpp:94-113; defaults 1, sqrt(0.5), 1e-4); get_gains: the proportional and integrator gains that follow;
 * get_freq: per stream (float[S] each) estimated_freq and the nu in use (floored to six decimals, = -estimated_freq).  step_mf_reset = Synchronizer_step_mf_cc::reset: the coarse
 * synchronizer, the matched filter's memory and the timing synchronizer.  dvbs2hip_sync_coarse_reset also clears the PLL.
 * dvbs2hip_sync_coarse_set_freq and dvbs2hip_sync_coarse_reset, host-only setters before the loop existed, now act on the per-stream state: when the loop ran last they
 * first bring that state back from the device (one small blocking copy on the handle's stream) and, like every entry that needs it on the host, return
 * DVBS2HIP_EUNSUPPORTED inside an open capture in that case.  Without a step_mf call on the handle they behave as before.
 * The handle's filter must have 81 symmetric taps (taps[i] == taps[80 - i], checked at create): otherwise step_mf returns DVBS2HIP_EUNSUPPORTED.
 * Graph capture: a task with a memory, the rule of the timing entries holds; the first call (it allocates and uploads) and the resets refuse an open capture. */
int dvbs2hip_sync_coarse_set_pll(dvbs2hip_t *h, int32_t pll_sps, float damping, float nbw);
int dvbs2hip_sync_coarse_get_gains(dvbs2hip_t *h, float *proportional, float *integrator);
int dvbs2hip_sync_coarse_get_freq(dvbs2hip_t *h, float *estimated_freq, float *nu);
int dvbs2hip_sync_step_mf_synchronize(dvbs2hip_t *h, const int32_t *DEL, const float *X_N1, float *MU, float *FRQ, float *PHS, float *Y_N1, int32_t *B_N1, int32_t n_frames);
int dvbs2hip_sync_step_mf_synchronize_dev(dvbs2hip_t *h, const int32_t *DEL, const float *X_N1, float *MU, float *FRQ, float *PHS, float *Y_N1, int32_t *B_N1, int32_t n_frames);
int dvbs2hip_sync_step_mf_reset(dvbs2hip_t *h);
/* The form of the coarse-frequency loop behind dvbs2hip_sync_step_mf_synchronize / _dev
 * DVBS2HIP_SMF_LANE (the default): one lane per stream walks rotation, the 81 taps, the timing step and the PLL for every sample; 64 streams share a wave.  A handle that
 * never calls this entry launches that kernel exactly as before the entry existed.
 * DVBS2HIP_SMF_WAVE: one wave per stream.  nu changes only in the PLL update on a pilot strobe, so rotation and matched filter are a feed-forward of the input in between:
 * the wave takes chunks of up to 64 samples, lane i rotates and filters sample i of the chunk with the nu in use, and only the timing step and the PLL then run sample by
 * sample.  When the PLL update at sample i of a chunk changes nu, samples 0 .. i are final, the chunk is cut there and what lay behind is rotated and filtered again from
 * the input with the new nu.  Every lane evaluates the lane form's expressions in the lane form's order: results and state are bit for bit the lane form's (and the CPU
 * twin's, tests/stepmf_twin.c; tests/stepmf_wave_twin.c states the chunked order on the CPU).  Five times faster than LANE with one stream and faster up to a few thousand; with a
 * full device of streams LANE, which shares a wave among 64 of them, has the higher throughput (results/coarse/README.md has both forms and where they cross).
 * The choice is a host-side field read at launch: it clears no state, no reset or set_streams changes it, and a handle may change form between any two calls.  It is
 * allowed inside an open capture; a recorded graph keeps the kernel it was recorded with, as with dvbs2hip_sync_timing_set_act.  Any other value: DVBS2HIP_EINVAL.
 * Every condition of the loop holds for both forms: 81 symmetric taps, two samples per symbol, DVBS2HIP_EUNSUPPORTED while the timing type is DVBS2HIP_STM_ULTRA. */
enum { DVBS2HIP_SMF_LANE = 0, DVBS2HIP_SMF_WAVE = 1 };
int dvbs2hip_sync_step_mf_set_kernel(dvbs2hip_t *h, int32_t kernel);

/* ------------------------------------------------------------------ N4: frame synchronizer
 * replaces: Synchronizer_frame_DVBS2_fast<R> (type "FAST", the factory default,
 * src/common/Factory/Module/Synchronizer_frame/Synchronizer_frame.cpp:71-72, .hpp:26-30) --
 * src/common/Module/Synchronizer/Synchronizer_frame/Synchronizer_frame_DVBS2_fast.cpp:
 *   synchronize1 (:132-150)  differential signal, correlators corr_SOF (25 taps) / corr_PLSC (64 taps)
 *   synchronize2 (:222-299)  cor_SOF delayed by 64, correlation metric, alpha-average, arg max -> delay,
 *                            variable output delay (Filter/Variable_delay/Variable_delay_cc_naive.cpp:56-79)
 *   synchronize  (:46-128)   both in one task
 * A call carries n_frames PL frames that are consecutive in time -- after dvbs2hip_set_streams(h, S > 1): S streams of
 * n_frames / S consecutive frames each, every stream with a state of its own -- and behaves per stream as that many calls of the
 * reference task with its n_frames = 1 (the reference's delay line re-reads its own output socket, so
 * its multi-frame form depends on what the socket held before; that case is not reproduced).  State
 * (correlator memories, reg_channel, corr_vec, delay lines, previous output frame) lives in the handle.
 *   X_N1: float[n_frames * 2*pl_frame]; cor_SOF, cor_PLSC, Y_N2: same size; DEL (delay), FLG (packet flag, may be
 *   NULL): int32_t[n_frames]; TRI (metric, may be NULL): float[n_frames] -- the sockets of Synchronizer_frame.hxx:40-81
 * set_params: alpha / trigger (defaults 0.9 / 30) and vec_width = mipp::N<float>() of the reference build
 * (default 8 = AVX2): the samples past the last full vector of a frame are not alpha-averaged (:284-285).
 * get_metric: _get_metric / _get_packet_flag (.hpp:59-60) after the last frame processed; with S streams, S entries each (float[S], int32_t[S]). */
int dvbs2hip_sync_frame_set_params(dvbs2hip_t *h, float alpha, float trigger, int32_t vec_width);
int dvbs2hip_sync_frame_reset(dvbs2hip_t *h);
int dvbs2hip_sync_frame_synchronize1(dvbs2hip_t *h, const float *X_N1, float *cor_SOF, float *cor_PLSC, int32_t n_frames);
int dvbs2hip_sync_frame_synchronize1_dev(dvbs2hip_t *h, const float *X_N1, float *cor_SOF, float *cor_PLSC, int32_t n_frames);
int dvbs2hip_sync_frame_synchronize2(dvbs2hip_t *h, const float *X_N1, const float *cor_SOF, const float *cor_PLSC, int32_t *DEL, int32_t *FLG,
                                     float *TRI, float *Y_N2, int32_t n_frames);
int dvbs2hip_sync_frame_synchronize2_dev(dvbs2hip_t *h, const float *X_N1, const float *cor_SOF, const float *cor_PLSC, int32_t *DEL, int32_t *FLG,
                                         float *TRI, float *Y_N2, int32_t n_frames);
int dvbs2hip_sync_frame_synchronize(dvbs2hip_t *h, const float *X_N1, int32_t *DEL, int32_t *FLG, float *TRI, float *Y_N2, int32_t n_frames);
int dvbs2hip_sync_frame_synchronize_dev(dvbs2hip_t *h, const float *X_N1, int32_t *DEL, int32_t *FLG, float *TRI, float *Y_N2, int32_t n_frames);
/* (round 5) CHAINED device form for a consumer of this library (Synchronizer_frame_DVBS2_fast.cpp:296-299 materializes Y_N2 only because the next task is a separate
 * module): the same synchronizer -- same DEL / FLG / TRI, same state for the next call -- but instead of the delayed copy it returns where each aligned frame STARTS:
 * SRC[f] (device table of n_frames device pointers, 8-byte aligned frames of 2 * pl_frame floats) points into X_N1 when the frame is one run of the input stream (the
 * delay did not move from frame f - 1: every frame in lock but the first and the last of a call) and into scratch of the handle otherwise.  X_N1 and the table must stay
 * untouched until their consumer -- dvbs2hip_rx_bb_located_dev, on the same handle and stream -- has run; the next synchronizer call reuses the scratch.  Bit-exact by
 * construction: the delay line only copies.                                                    */
int dvbs2hip_sync_frame_locate_dev(dvbs2hip_t *h, const float *X_N1, int32_t *DEL, int32_t *FLG, float *TRI, const float **SRC, int32_t n_frames);
int dvbs2hip_sync_frame_get_metric(dvbs2hip_t *h, float *max_corr, int32_t *packet_flag);

/* ------------------------------------------------------------------ N4: fine frequency / phase synchronizers
 * replace: Synchronizer_freq_fine::synchronize (sockets X_N1, FRQ, PHS, Y_N2: Synchronizer_freq_fine.hxx:32-47) of
 *   Synchronizer_Luise_Reggiannini_DVBS2_aib -- src/common/Module/Synchronizer/Synchronizer_freq/Synchronizer_freq_fine/
 *     Synchronizer_Luise_Reggiannini_DVBS2_aib.cpp:93-167 (autocorrelation of the pilot blocks, damped by lr_alpha from
 *     frame to frame -- default 0.999, Factory/Module/Synchronizer_freq_fine/Synchronizer_freq_fine.hpp:25 -- then the
 *     frame is rotated by the estimated frequency); _reset :170-176
 *   Synchronizer_freq_phase_DVBS2_aib -- .../Synchronizer_freq_phase_DVBS2_aib.cpp:44-112 (phase of every pilot block,
 *     unwrapped, least-squares line -> frequency and phase, rotation of the frame); stateless
 * Input = PL-DESCRAMBLED frames (the RX mains run them after Scrambler_PL::descramble).
 *   X_N1, Y_N2: float[n_frames * 2*pl_frame]; FRQ, PHS: float[n_frames] (may be NULL)                         */
int dvbs2hip_sync_lr_synchronize(dvbs2hip_t *h, const float *X_N1, float *FRQ, float *PHS, float *Y_N2, int32_t n_frames);
int dvbs2hip_sync_lr_synchronize_dev(dvbs2hip_t *h, const float *X_N1, float *FRQ, float *PHS, float *Y_N2, int32_t n_frames);
int dvbs2hip_sync_lr_set_alpha(dvbs2hip_t *h, float alpha);
int dvbs2hip_sync_lr_reset(dvbs2hip_t *h);
/* L&R runs its serial recurrence and the rotation in ONE launch: the rotating workgroups wait for workgroup 0's estimates, which assumes that the
 * dispatcher places workgroup 0 first ("L&R dispatch order").  A workgroup that waits longer than one second of wall-clock time
 * drops its stores and sets an error word; the host-socket form repeats the rotation before it returns, the _dev form when dvbs2hip_synchronize
 * is called (it returns DVBS2HIP_EHIP only if the repeat itself fails).  This counts the launches that needed the repeat (0 on every box so far). */
int dvbs2hip_sync_lr_timeouts(dvbs2hip_t *h, int32_t *n_launches_repeated);
int dvbs2hip_sync_freq_phase_synchronize(dvbs2hip_t *h, const float *X_N1, float *FRQ, float *PHS, float *Y_N2, int32_t n_frames);
int dvbs2hip_sync_freq_phase_synchronize_dev(dvbs2hip_t *h, const float *X_N1, float *FRQ, float *PHS, float *Y_N2, int32_t n_frames);

/* ------------------------------------------------------------------ PLS decoder (extension: the reference has no such task, it takes the MODCOD from the command line)
 * inverts: Framer<B>::generate_plh -- src/common/Module/Framer/Framer.hxx:97-196: seven bits b0..b6 times the 7 x 32 matrix G (row 0 the extension row, rows 1-5
 *   the Walsh rows, row 6 all ones), every coded bit sent twice as y[2i] = c[i], y[2i+1] = c[i] ^ p (the framer always sends p = 1), XOR the 64-bit PLS scrambler,
 *   pi/2-BPSK, times j when b0 = 1, behind the 26 SOF symbols.
 * Per aligned PL frame, from its 90 header symbols r[k]:
 *   PLS: int32_t[n_frames], V = b0 128 + b1 64 + b2 32 + b3 16 + b4 8 + b5 4 + b6 2 + p -- V & 127 is the standard's MODCOD * 4 + TYPE (pilots in bit 0), bit 7 the
 *        extension bit; QPSK-S_8/9 with pilots is 43.  V = the one of the 256 headers H with the largest |sum_k r[k] conj(H[k])| over all 90 symbols (maximum
 *        likelihood for an unknown constant phase; the SOF tells a code word from its complement).  Of equal metrics the smallest V wins.
 *   MET: float[n_frames] (may be NULL), that metric; ENE: float[n_frames] (may be NULL), sum_k |r[k]|^2 -- MET / sqrt(90 ENE) is the normalised correlation.
 *   X_N1: float[n_frames * 2*pl_frame], aligned frames: the frame synchronizer's Y_N2, before or after dvbs2hip_pl_descramble (the scrambler copies the header,
 *        Scrambler_PL.hxx:63).  The located form reads frame f at SRC[f] instead: the table dvbs2hip_sync_frame_locate_dev fills (device pointers, 8-byte
 *        aligned), same results bit for bit as the plain form on the same samples.
 * Stateless: frames of S streams in one call are just frames.  n_frames in [1, max_frames].  The _dev forms are stream-ordered and may be recorded in a graph.
 * fp32 in an order of its own (dvbs2_amd/csrc/k_pls.hip): bit-exact with nothing, held to a float64 search over the 256 headers by tests/test_pls_gpu.py.
 * expected: the V of the handle's own configuration (cfg.pls, p = 1), what every frame of a matching stream decodes to.
 * describe: no handle; the name of the MODCOD of the library's table whose pls row is value >> 1 ("" when there is none) and pilots = value & 1 (may be NULL);
 *   DVBS2HIP_EINVAL for a value outside 0..255.                                                    */
int dvbs2hip_pls_decode(dvbs2hip_t *h, const float *X_N1, int32_t *PLS, float *MET, float *ENE, int32_t n_frames);
int dvbs2hip_pls_decode_dev(dvbs2hip_t *h, const float *X_N1, int32_t *PLS, float *MET, float *ENE, int32_t n_frames);
int dvbs2hip_pls_decode_located_dev(dvbs2hip_t *h, const float *const *SRC, int32_t *PLS, float *MET, float *ENE, int32_t n_frames);
int dvbs2hip_pls_expected(dvbs2hip_t *h, int32_t *value);
int dvbs2hip_pls_describe(int32_t value, char *name, int32_t name_len, int32_t *pilots);

/* ------------------------------------------------------------------ PLHEADER search (extension: the reference has no such task; built on the PLS decoder above)
 * What an unknown constant-coding-and-modulation stream is and where its PL frames start, from symbols at one sample per symbol, without a MODCOD being given.
 * X: float[2 * n_sym], n_sym complex symbols, 8-byte aligned and no more; 90 <= n_sym <= DVBS2HIP_PLS_SCAN_MAX_SYM (DVBS2HIP_EINVAL otherwise).  There are
 *   K = n_sym - 89 offsets.  Neither call depends on the handle's MODCOD or on max_frames.
 * scan: PLS: int32_t[K], MET: float[K] (may be NULL), ENE: float[K] (may be NULL).  Output k is what dvbs2hip_pls_decode_dev returns for a frame that starts at
 *   X + 2 k, bit for bit (dvbs2_amd/csrc/k_pls_search.hip builds the same sums in the same order with the lanes across offsets; tests/test_pls_search_gpu.py).
 * search: LEN: int32_t[256], the PL frame length in symbols that PLS value V implies, or 0 when V is not a candidate; entries below 90 count as 0.  A host pointer in
 *   the host form, a device pointer in the _dev form.  NULL: the library's own table, dvbs2hip_pls_frame_symbols(V) for V = 0 .. 255, uploaded once per handle.
 *   RES: int32_t[4] = {OFFSET, VALUE, COUNT, SLOTS}; SCORE: one float.  With (PLS, MET, ENE) the scan's outputs, all arithmetic fp32, each operation rounded once:
 *     q[k] = (MET[k] * MET[k]) / (90 * ENE[k]), and 0 when ENE[k] = 0.  By Cauchy-Schwarz q <= 1: the share of the window's energy that the best header explains,
 *       so a gain in front changes nothing.
 *     Offset k is a start when L = LEN[PLS[k]] > 0 and k < L.
 *     A start's slots are k_j = k + j L < K, j = 0 .. J - 1.
 *     Its score is C = sum over j ascending of q[k_j] where PLS[k_j] = PLS[k], and of 0 where it is not; the sum is serial from 0.  COUNT is the number of slots that
 *       match (slot 0 always does).
 *     The winner has the largest C; among equal C the smallest k.
 *     OFFSET = k, VALUE = PLS[k], COUNT, SLOTS = J, SCORE = C.  OFFSET = -1 and the other outputs zero when no offset is a start.
 *   A caller accepts the result or not (dvbs2_amd.params.find_modcod: COUNT >= 2 and SCORE >= q_min SLOTS; results/pls_search/README.md has q_min's measurement).
 * frame_symbols: no handle; pl_frame of the MODCOD of the library's table whose PLS value (pilots on: the only frames the library builds) is `value`, 0 when there is
 *   none -- an even value, a value outside 0..255, a row the table does not have.
 * The search is coherent over the header's 90 symbols and tolerates what the PLS decoder tolerates (a residual carrier of 1e-3 cycles per symbol at 0 dB); it assumes
 * frames of one length laid back to back (the PLHEADER walk below goes from header to header), and knows nothing of dummy frames.
 * The _dev forms take device addresses, are stream-ordered and make no host round trip: the scan one launch, the search three (scan, chain scores, reduction), none of
 * which waits on another workgroup.  search_dev keeps (PLS, MET, ENE) and the reduction's partial results in the handle's workspace, 12 bytes per offset: it may be
 * recorded in a graph after one call of the same n_sym (and LEN = NULL, if that is used) outside the capture, which allocates.                                       */
#define DVBS2HIP_PLS_SCAN_MAX_SYM (1 << 24)
int dvbs2hip_pls_scan(dvbs2hip_t *h, const float *X, int32_t n_sym, int32_t *PLS, float *MET, float *ENE);
int dvbs2hip_pls_scan_dev(dvbs2hip_t *h, const float *X, int32_t n_sym, int32_t *PLS, float *MET, float *ENE);
int dvbs2hip_pls_search(dvbs2hip_t *h, const float *X, int32_t n_sym, const int32_t *LEN, int32_t *RES, float *SCORE);
int dvbs2hip_pls_search_dev(dvbs2hip_t *h, const float *X, int32_t n_sym, const int32_t *LEN, int32_t *RES, float *SCORE);
int dvbs2hip_pls_frame_symbols(int32_t value);

/* ------------------------------------------------------------------ PLHEADER walk (extension: the reference has no such task; built on the PLS decoder above)
 * A stream whose MODCOD changes from one PL frame to the next (VCM / ACM): from a header at symbol `start`, along the chain of frames whose lengths their own headers
 * give, where every frame starts and what it is, and the frames grouped by PLS value as pointer tables that go into the located decoders of one handle per MODCOD.
 * X: as in the search -- float[2 * n_sym], 8-byte aligned, 90 <= n_sym <= DVBS2HIP_PLS_SCAN_MAX_SYM.  0 <= start <= n_sym and 1 <= max_out; anything else is
 *   DVBS2HIP_EINVAL, and the handle stays usable.  The call depends neither on the handle's MODCOD nor on max_frames.
 * LEN: int32_t[256] as in the search (a host pointer in the host form, a device pointer in the _dev form, NULL: the library's own table).  LEN'[V] = LEN[V], and 0
 *   where LEN[V] is below 90 or no multiple of 18.  Every DVB-S2 PL frame length, 90 (S + 1) + 36 P, is a multiple of 18, so every header of a chain sits at start + 18 i.
 * For an offset c with c + 90 <= n_sym, (PLS, MET, ENE)(c) are what dvbs2hip_pls_decode_dev returns for a frame that starts at X + 2 c, bit for bit, and
 *   q(c) = (MET * MET) / (90 * ENE) in fp32, each operation rounded once, 0 when ENE = 0: the search's q.
 * The walk: c = start, j = 0, then in this order
 *   1. c + 90 > n_sym: stop, END.
 *   2. V = PLS(c), L = LEN'[V].
 *   3. L = 0, or not q(c) >= q_min: stop, LOST.
 *   4. c + L > n_sym: stop, END (the header was seen, the frame is not all there).
 *   5. j = max_out: stop, FULL.
 *   6. OFF[j] = c, VAL[j] = V, Q[j] = q(c); c += L, j += 1; again from 1.
 *   In every stop NEXT = c: the symbol from which the caller carries the tail into its next buffer, or from which it acquires again.
 * RES: int32_t[4] = {N, NEXT, STATUS, 0}, N = j, STATUS DVBS2HIP_PLS_WALK_END = 0, _LOST = 1, _FULL = 2.  OFF, VAL: int32_t[max_out], Q: float[max_out].
 * CNT: int32_t[256], the frames per value.  IDX: int32_t[max_out] and SRC: max_out device pointers (_dev form only; may be NULL): the frames grouped by value ascending,
 *   in stream order within a value -- IDX[g] = j and SRC[g] = X + 2 OFF[j].  Value v's group begins at the sum of CNT[u], u < v, and goes as it stands into
 *   dvbs2hip_rx_bb_located_dev / dvbs2hip_estimate_pilots_located_dev of a handle of that MODCOD.  Entries at and past N are undefined.
 * The _dev form takes device addresses, is stream-ordered and makes no host round trip; no workgroup waits on another and nothing spins.  The PLS decoder runs on the
 *   candidates start + 18 i alone; the chain is then resolved by one lane where it can only be short, and otherwise by pointer doubling over the candidates, about
 *   2 log2(frames) small launches of integer arithmetic whose result does not depend on any order (dvbs2_amd/csrc/k_pls_walk.hip, results/pls_walk/README.md).  The
 *   candidates' (PLS, MET, ENE) and the jump table live in the handle's workspace: the call may be recorded in a graph after one call of the same n_sym and max_out
 *   (and LEN = NULL, if that is used) outside the capture, which allocates for any start.  The host form stages X and returns everything but SRC.
 * Acquisition -- which `start` -- is the caller's: dvbs2_amd.params.find_vcm_start picks it from one dvbs2hip_pls_scan of a stream's head.  Pilot-less frames and
 *   carrier recovery across MODCODs are not provided.                                                    */
#define DVBS2HIP_PLS_WALK_END 0
#define DVBS2HIP_PLS_WALK_LOST 1
#define DVBS2HIP_PLS_WALK_FULL 2
int dvbs2hip_pls_walk(dvbs2hip_t *h, const float *X, int32_t n_sym, int32_t start, const int32_t *LEN, float q_min, int32_t max_out, int32_t *OFF, int32_t *VAL, float *Q,
                      int32_t *IDX, int32_t *CNT, int32_t *RES);
int dvbs2hip_pls_walk_dev(dvbs2hip_t *h, const float *X, int32_t n_sym, int32_t start, const int32_t *LEN, float q_min, int32_t max_out, int32_t *OFF, int32_t *VAL,
                          float *Q, const float **SRC, int32_t *IDX, int32_t *CNT, int32_t *RES);

/* ------------------------------------------------------------------ pilot-aided noise estimator (extension: the reference has no such task; its only estimator is
 * Estimator_DVBS2, dvbs2hip_estimate above, whose Se = sqrt(|2 m2^2 - m4|) takes every constellation point to have the same modulus: on 16APSK it never reads above
 * about 8.8 dB of Es/N0 and on 32APSK it stops near 5 dB, so sigma comes out 2 to 2.8 times too large)
 * Per aligned PL frame y[n] of pl_frame symbols, from the L = 90 + 36 N_pilots symbols the receiver knows: the header at [0, 90), which carries the header of the
 * handle's framer (cfg.pls, pairing bit 1), and pilot block b = 1..N_pilots at [90 + 1440 b + 36 (b - 1), +36), which carries (1 + j) / sqrt(2).  With p[k] those
 * unit-modulus values and y[k] the received ones:
 *   c = (1/L) sum_k y[k] conj(p[k])
 *   N = sum_k |y[k] - c p[k]|^2 / (L - 1)          (noise power per complex symbol; the residual form: nothing small is the difference of two large numbers)
 *   A = |c|^2,  S = A - N / L,  Es_N0 = 10 log10(S / N)
 *   S <= 0: Es_N0 = -100; N = 0, or a ratio of 100 dB and more: Es_N0 = +100 (an fp32 frame without noise leaves N near 1e-14 A).
 *   SIG = sqrt(1 / (2 10^(Es_N0 / 10))), Eb_N0 = Es_N0 - 10 log10(code rate x bits per symbol): the M2M4 task's expressions, and its sockets -- SIG, Eb_N0, Es_N0:
 *   float[n_frames], each may be NULL.
 * scrambled = 1: X_N1 is what the frame synchronizer delivers (header copied, pilots PL-scrambled); every pilot sample is first descrambled as dvbs2hip_pl_descramble
 *   does it for its position (a swap or a sign change, exact).  scrambled = 0: X_N1 is already PL-descrambled (what L&R and the pilot-phase synchronizer produce).  The
 *   two give the same results bit for bit.
 * X_N1: float[n_frames * 2*pl_frame]; the host form stages only the known symbols' bytes.  The located form reads frame f at SRC[f] instead: the table
 *   dvbs2hip_sync_frame_locate_dev fills (device pointers, 8-byte aligned), same results bit for bit as the plain form on the same samples.  SIG of a _dev form is a
 *   device array that goes straight into dvbs2hip_rx_bb_dev / dvbs2hip_rx_bb_located_dev as sigma_in.
 * The estimate is coherent over the frame: a constant phase does not move it, a residual carrier lowers S.  It belongs behind the fine synchronizers, or on a baseband
 *   loop with no carrier error; removing the carrier is not this task's job.
 * set_alpha(alpha), 0 <= alpha < 1, default 0 = every frame on its own and no state.  alpha > 0: the handle keeps (Abar, Nbar) per stream of dvbs2hip_set_streams
 *   (stream s = frames [s F/S, (s+1) F/S); n_frames has to be a multiple of S); a stream's first frame after _reset sets Abar = A, Nbar = N, every later one does
 *   x = alpha x + (1 - alpha) v in fp32, frames in order, and S and the outputs are formed from Abar, Nbar.  dvbs2hip_reset and dvbs2hip_set_streams reset this state too.
 * n_frames in [1, max_frames].  The _dev forms are stream-ordered and may be recorded in a graph (alpha > 0: after one call outside the capture, which allocates the state).
 * fp32 in an order of its own (dvbs2_amd/csrc/k_est_pilots.hip): bit-exact with nothing, held to float64 (tests/est_pilots_ref.py) at 1e-4 max(1, |x|).                  */
int dvbs2hip_estimate_pilots(dvbs2hip_t *h, const float *X_N1, int32_t scrambled, float *SIG, float *Eb_N0, float *Es_N0, int32_t n_frames);
int dvbs2hip_estimate_pilots_dev(dvbs2hip_t *h, const float *X_N1, int32_t scrambled, float *SIG, float *Eb_N0, float *Es_N0, int32_t n_frames);
int dvbs2hip_estimate_pilots_located_dev(dvbs2hip_t *h, const float *const *SRC, int32_t scrambled, float *SIG, float *Eb_N0, float *Es_N0, int32_t n_frames);
int dvbs2hip_estimate_pilots_set_alpha(dvbs2hip_t *h, float alpha);
int dvbs2hip_estimate_pilots_reset(dvbs2hip_t *h);

/* ------------------------------------------------------------------ BBFRAME layer (extension: the reference has no such task; its chain begins and ends in K_bch
 * anonymous bits per frame.  EN 302 307-1 clause 5.1, mode adaptation, for one packetised stream)
 * Bit i of a frame is element i of the int32_t[K_bch] socket; byte k of a frame is bits 8k .. 8k+7, bit 8k the byte's bit 7; multi-bit fields most significant bit first.
 * BBFRAME = BBHEADER (80 bits) | DATA FIELD (DFL bits) | K_bch - 80 - DFL zero bits; it then goes through the BB scrambler (dvbs2hip_bb_scramble, dvbs2hip_tx_bb's info_in).
 * BBHEADER: MATYPE-1, MATYPE-2, UPL (2 bytes, the user packet length in bits), DFL (2 bytes), SYNC, SYNCD (2 bytes: bits from the start of the data field to the first
 *   packet that starts in it, 65535 = none does), CRC-8 of these nine bytes.  CRC-8: g(x) = x^8 + x^7 + x^6 + x^4 + x^2 + 1, register 0 at the start, nothing reflected, no
 *   final xor ("123456789" -> 0xBC).
 * Packets: UPLB = UPL / 8 bytes each, byte 0 the sync byte; on air the CRC-8 of a packet's other UPLB - 1 bytes stands in the place of the NEXT packet's sync byte (its
 *   "slot"; the very first slot carries 0), and the byte stream is cut into data fields with no regard for packet borders.
 * set_params(matype1, matype2, upl_bits, sync, mark_tei): defaults 0xF2 (transport stream, single stream, CCM, roll-off 0.20), 0, 1504, 0x47, 0.  upl_bits has to be a
 *   multiple of 8 in [16, K_bch - 80]: DVBS2HIP_EUNSUPPORTED otherwise (continuous streams, UPL = 0, are not provided).  It resets both tasks.
 * reset: both tasks' state and the counters to zero; a no-op on a handle that has not used the layer; dvbs2hip_reset calls it.
 * get_stats: uint64_t[5] = {frames taken, frames dropped, packets with a right CRC-8, packets with a wrong one, bytes discarded}, since the last reset (it synchronises).
 *
 * build: the next n_bytes bytes UP of the packet stream -> U_K, int32_t[n_frames * K_bch], with D = (K_bch - 80) / 8 and (n_frames - 1) D < n_bytes <= n_frames D
 *   (DVBS2HIP_EINVAL otherwise): all frames but the last are full, the last one takes the rest (DFL = 8 rest) and is padded.  The task keeps the position in the
 *   current packet and the CRC-8 registers from call to call, so a stream may be cut into calls anywhere.  The sync bytes of UP are not looked at.
 *
 * parse: V_K, int32_t[n_frames * K_bch], descrambled frames; VALID, int8_t[n_frames] or NULL: 0 = this frame is not to be trusted (e.g. the BCH flag)
 *   -> UP: the packets, contiguous, in stream order, capacity * UPLB bytes; STATUS: uint8_t[capacity], 0 = the packet's CRC-8 is right, 1 = wrong; N_OUT: int32_t[1], how
 *   many; HDR: int32_t[n_frames * 8] or NULL, per frame {status, MATYPE-1 << 8 | MATYPE-2, UPL, DFL, SYNC, SYNCD, CRC-8 received, CRC-8 computed}.
 *   capacity = dvbs2hip_bbframe_max_packets(h, n_frames) = floor((n_frames D + UPLB - 1) / UPLB); N_OUT never exceeds it.
 *   Frame status: 3 VALID[f] == 0; else 1 the header's CRC-8 is wrong; else 2 a field is refused (UPL or SYNC not the configured one, DFL > K_bch - 80 or not a multiple of
 *   8, SYNCD not a multiple of 8, SYNCD >= DFL and not 65535); else 0, taken.
 *   The packets are those of this rule, applied to the frames in order, `buf` (the pending packet) and `have` carried from call to call:
 *     status != 0:                     discard buf (count its bytes); have = false; next frame
 *     df = the DFL / 8 bytes of the data field
 *     SYNCD == 65535:                  discard buf and df (count both); have = false; next frame
 *     s = SYNCD / 8
 *     have and len(buf) + s == UPLB:   emit buf + df[:s], its slot is df[s]
 *     otherwise:                       discard buf and df[:s] (count both)
 *     for start = s, s + UPLB, ... while start + UPLB < len(df):   emit df[start : start + UPLB], its slot is df[start + UPLB]
 *     buf = df[last start :] (1 .. UPLB bytes: a packet that ends on df's last byte waits for its slot); have = true
 *   emit: byte 0 becomes SYNC; STATUS = the CRC-8 over bytes 1 .. UPLB - 1 differs from the slot's byte; with mark_tei, UPL = 1504 and STATUS = 1, bit 7 of byte 1 (a
 *   transport packet's transport_error_indicator) is set.
 *   A frame without a packet start (SYNCD = 65535) discards what is pending instead of extending it.  That is deliberate: what a frame emits then depends on its own
 *   header and the one before it only, so the device counts the packets of all frames at once, places them with one scan, and copies and checks every packet on its own.
 *   While UPLB <= D every full data field holds a packet start, so only a short last frame that carries nothing but a packet's tail is lost this way.
 *
 * rx_bb_up: dvbs2hip_rx_bb_dev into a bit buffer of the handle, then parse with VALID = NULL, in one call; cwd_ldpc / cwd_bch: int8_t[n_frames], may be NULL.  The host
 *   form copies back the packets, statuses, headers and flags only: about K_bch / 8 bytes of a frame where dvbs2hip_rx_bb returns 4 K_bch.
 *
 * n_frames in [1, max_frames].  The _dev forms take device addresses (U_K, V_K 16-byte aligned), are stream-ordered, make no host round trip and a number of launches
 * that does not depend on n_frames; parse_dev and rx_bb_up_dev may be recorded in a graph after one call outside the capture (which allocates), and as with every task
 * that keeps a memory each replay starts from the state of the moment of recording.  Integer arithmetic throughout: bit-exact with tests/bbframe_ref.py.
 * Not provided: multiple input streams, ISSY, null-packet deletion, ACM, continuous generic streams.                                                                 */
int dvbs2hip_bbframe_set_params(dvbs2hip_t *h, int32_t matype1, int32_t matype2, int32_t upl_bits, int32_t sync, int32_t mark_tei);
int dvbs2hip_bbframe_reset(dvbs2hip_t *h);
int dvbs2hip_bbframe_get_stats(dvbs2hip_t *h, uint64_t *stats);
int dvbs2hip_bbframe_max_packets(dvbs2hip_t *h, int32_t n_frames, int32_t *capacity);
int dvbs2hip_bbframe_build(dvbs2hip_t *h, const uint8_t *UP, int64_t n_bytes, int32_t *U_K, int32_t n_frames);
int dvbs2hip_bbframe_build_dev(dvbs2hip_t *h, const uint8_t *UP, int64_t n_bytes, int32_t *U_K, int32_t n_frames);
int dvbs2hip_bbframe_parse(dvbs2hip_t *h, const int32_t *V_K, const int8_t *VALID, uint8_t *UP, uint8_t *STATUS, int32_t *N_OUT, int32_t *HDR, int32_t n_frames);
int dvbs2hip_bbframe_parse_dev(dvbs2hip_t *h, const int32_t *V_K, const int8_t *VALID, uint8_t *UP, uint8_t *STATUS, int32_t *N_OUT, int32_t *HDR, int32_t n_frames);
int dvbs2hip_rx_bb_up(dvbs2hip_t *h, const float *pl_frames, const float *sigma_in, uint8_t *UP, uint8_t *STATUS, int32_t *N_OUT, int32_t *HDR, int8_t *cwd_ldpc, int8_t *cwd_bch,
                      int32_t n_frames);
int dvbs2hip_rx_bb_up_dev(dvbs2hip_t *h, const float *pl_frames, const float *sigma_in, uint8_t *UP, uint8_t *STATUS, int32_t *N_OUT, int32_t *HDR, int8_t *cwd_ldpc, int8_t *cwd_bch,
                          int32_t n_frames);

/* ------------------------------------------------------------------ measurement
 * Per-kernel device time, measured with hipEvents recorded on the handle's stream around
 * each launch while timing is enabled (the equivalent of `--sim-stats`,
 * TX_RX_BB/main.cpp:110,170-178).                                                    */
enum { DVBS2HIP_K_LDPC = 0, DVBS2HIP_K_BCH = 1, DVBS2HIP_K_DEMAP = 2, DVBS2HIP_K_FIR = 3,
       DVBS2HIP_K_FRONT = 4, DVBS2HIP_K_MISC = 5, DVBS2HIP_K_COUNT = 6 };
int dvbs2hip_timing_enable(dvbs2hip_t *h, int32_t on);
int dvbs2hip_timing_reset(dvbs2hip_t *h);
/* synchronises, then returns the summed device ms and the number of launches of kernel k */
int dvbs2hip_timing_get(dvbs2hip_t *h, int32_t k, double *total_ms, int64_t *n_launches);
/* what a plain device-to-device copy reaches on this GPU with a kernel of this library (16 bytes per lane and access; the best of 1 / 4 accesses
 * in flight per lane, plain / non-temporal): read + written bytes over the hipEvent time of `reps` copies of `bytes` bytes in scratch memory, in GB/s.  A measurement aid for the roofline figures (bench.py: `roofline.hbm_copy_GBps_measured`); the
 * reference has no counterpart.                                                        */
int dvbs2hip_device_copy_bandwidth(dvbs2hip_t *h, size_t bytes, int32_t reps, double *GBps);
/* device memory helpers so non-HIP hosts (ctypes, cgo, JNI) can own device buffers */
int dvbs2hip_malloc(dvbs2hip_t *h, void **dptr, size_t bytes);
int dvbs2hip_free(dvbs2hip_t *h, void *dptr);
int dvbs2hip_memcpy_h2d(dvbs2hip_t *h, void *dst, const void *src, size_t bytes);
int dvbs2hip_memcpy_d2h(dvbs2hip_t *h, void *dst, const void *src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* DVBS2HIP_H */
