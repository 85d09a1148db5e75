// Internal declarations shared by the HIP translation units of libdvbs2hip.so.
// Nothing here is part of the ABI (include/dvbs2hip.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/dvbs2hip.h"
#include "ldpc_layer_table.h"
#include "rx_dispatch.h"

namespace dvbs2 {

// e^x and ln x on the hardware transcendental units, ONE v_exp_f32 / v_log_f32 plus a multiply each.  HIP's __expf / __logf
// wrap the same instructions in a range check and a rescale for denormal results (8 instructions instead of 2); the
// arguments here (exp of a non-positive number, log of a sum >= 1 or of a sum of such exponentials) do not need that:
// a result below the smallest normal number flushes to zero, which is what the formulas treat it as.
#if defined(__HIPCC__)
__device__ __forceinline__ float hw_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
__device__ __forceinline__ float hw_log(float x) { return __builtin_amdgcn_logf(x) * 0.693147180559945309f; }
#endif

// ---------------------------------------------------------------- LDPC (a1)
// One slot of a QC layer = one circulant: variable = group element (t - t0) mod 360.
// Packed in ONE dword so a whole layer (<= 27 entries) is preloaded into SGPRs by a few wide
// scalar loads:  bits 0..8 circulant shift t0 | bits 9..16 slot of the bit-group in its store
// (word offset = 360 * slot) | bit 17 store is LDS | bit 18 edge absent for t == 0 |
// bits 19..20 conflict level | bit 21 padding entry (no edge).
typedef uint32_t LdpcEntry;
enum { LE_T0_MASK = 0x1FF, LE_SLOT_SHIFT = 9, LE_SLOT_MASK = 0xFF, LE_LDS = 1u << 17, LE_MASK0 = 1u << 18,
       LE_LVL_SHIFT = 19, LE_LVL_MASK = 3, LE_NULL = 1u << 21 };

struct LdpcGroup {    // where the 360 posteriors of one bit-group live
    uint32_t base;
    uint32_t lds;     // 1 = LDS, 0 = per-frame global workspace
};

constexpr int LDPC_Z = 360;          // DVB-S2 parallelism factor
constexpr int TX_BCH_SEG = 16;       // segments (lanes) per frame of the TX BCH encoder (k_tx.hip, host-made shift table): 32 / 64 help 512-frame calls (61 -> 46 / 41 us) and cost 4096-frame ones (0.754 -> 0.768 / 0.812 ms per TX)
constexpr int LDPC_THREADS = 384;    // 6 wavefronts, 360 active lanes
constexpr int LDPC_MAX_SLOTS = 27;   // 27 sign bits + 5 index bits = one packed dword

struct LdpcKParams {
    const float *llr;        // [F][N]
    int32_t *bits;           // [F][K]            (may be null)
    uint32_t *packed;        // [F][K/32 words]   (may be null) packed hard decisions, bit i of word w = info bit 32 w + i
    int8_t *cwd;             // [F]               (may be null)
    float *post;             // [F][N] natural    (may be null)
    int32_t *ites;           // [F]               (may be null)
    // fused chain (k_ldpc_wg8.hip): the first K_info hard decisions XOR the BB descrambling sequence, one int32 per bit, straight
    // into the chain's output socket -- what the BCH stage would write for a frame it does not have to correct
    int32_t *info_out;       // [F][K_info]       (may be null)
    const uint32_t *info_prbs;  // PRBS by (row g, wave w): 64-bit word [g * 6 + w], bit l = PRBS bit 360 g + 64 w + l (zero from K_info on); wave-uniform scalars
    int32_t K_info;
    // (round 5) fused chain, BCH verification inside the LDPC kernel: a frame is a BCH codeword iff r(x) mod g(x) = 0.  Bit t of information row g is the coefficient
    // of x^(360 (G - 1 - g)) x^(359 - t): each lane XORs the row's factor A_g into its accumulator for every set hard decision it outputs, the wave applies the lanes'
    // factors once per frame (k_ldpc_wg8.hip, fold_syn).  The BCH stage then runs only over the flagged frames.
    const uint32_t *syn_tab;    // [syn_rows][8]: per row in STORAGE order (the order k_ldpc_wg8.hip emits the rows in: LDS rows, global rows, register slots) {byte offset 1440 g of the row in the int32
                                // socket (0x7FFFF000: an empty register slot), 1 = the last information row, A_g[0 .. 5] = x^(360 (n_info - 1 - g)) mod g(x)}, then [LDPC_SYN_RED][syn_words]: x^k mod g(x),
                                // little-endian 32-bit words; or null (no verification)
    const uint32_t *info_prbs_s;   // [syn_rows][LDPC_AT_LANES]: bit k of entry [ks][t] = the BB descrambler's bit of information bit 360 g + t, g the row emitted at storage position ks + k (k < 16)
    int32_t syn_words;          // 4 (deg g <= 128) or 6 (<= 192)
    int32_t syn_rows;           // rows the kernel emits (information rows + empty register slots)
    uint8_t *bch_flag;          // [F]: 1 = remainder not zero (the BCH stage decodes this frame), 0 = codeword
    int8_t *cwd_bch;            // [F] or null: the BCH stage's CWD flag, written (1) for a frame whose remainder is zero
    float *gwork;            // [grid][gwork_words] per-workgroup global workspace
    const LdpcEntry *entries;  // [q][deg_max_padded]
    const int32_t *layer_deg;  // [q]
    const int32_t *layer_lvl;  // [q] max conflict level in the layer
    const LdpcGroup *groups;   // [n_groups] info groups then parity groups
    int32_t N, K, M, q, n_info, n_groups;
    int32_t ent_stride;      // entries per layer in `entries`
    int32_t lds_post_words;  // LDS words used by posteriors
    int32_t glb_post_words;  // global words per frame used by posteriors
    int32_t gwork_words;     // global words per frame in total (posteriors + c2v state)
    int32_t n_frames, n_ite, early_stop;
    float alpha;
    const uint32_t *order;        // queue position -> frame index (n_frames entries), or null: frames in index order (k_ldpc_wg8.hip; built by frame_order_launch)
    float spa_cap;                // sum-product, exact check node: |c->v| is clipped to this (LDPC_SPA_CAP: the reference's results; +inf: no clip)
    int32_t inf_row;           // fast path: byte offset of the +inf row (padded layers) or -1
    uint32_t *cu_ctr;          // 8-wave workgroups: per-CU arrival counter (zeroed before the launch) or null
    struct {                   // k_ldpc_wg8.hip
        const uint32_t *tab;   // the layer tables, then the row-keeping waves' swaps (LdpcPlan::w8_tab; layout: ldpc_layer_table.h)
        const uint32_t *atab;  // per-lane address table (LdpcPlan::w8_atab) or null
        const uint32_t *rows;  // the image's rows in storage order, the parity groups' places, the register slots' rows (LdpcPlan::w8_rows; sections: ldpc_layer_table.h)
        uint32_t st_base;      // byte offset of the packed c->v state in the workgroup's global slot
        uint32_t lds_junk;     // byte offset of the write-only LDS row (the +inf row of padded codes follows it)
        int32_t lds_bytes, pad;
        int32_t nl_info, nl, ng_info, ng;
    } w8;
};

struct LdpcPlan {             // host-side description, built once per handle
    int N = 0, K = 0, M = 0, q = 0, n_info = 0, n_groups = 0, E = 0;
    int deg_max = 0, ent_stride = 0;
    int lds_groups = 0;
    bool c2v_lds = false, hybrid = false;
    int lds_post_words = 0, glb_post_words = 0, gwork_words = 0;
    size_t lds_bytes = 0;
    int grid_max = 1;         // persistent grid: resident workgroups on the device
    int n_cus = 256;          // compute units of the device (k_ldpc_nat.hip: the natural order's workgroup shape by batch size)
    std::vector<LdpcEntry> entries;
    std::vector<int32_t> layer_deg, layer_lvl;
    std::vector<LdpcGroup> groups;
    // device copies
    LdpcEntry *d_entries = nullptr;
    int32_t *d_layer_deg = nullptr, *d_layer_lvl = nullptr;
    LdpcGroup *d_groups = nullptr;
    // regular-code fast path (k_ldpc_wg8.hip): every layer has exactly fast_deg slots
    bool fast = false;
    bool spa = false;             // sum-product check node: per-edge fp32 messages instead of the packed min-sum state
    int spa_rule = 0;             // 0: not sum-product, 1: exact (complement-product domain), 2: AFF3CT's saturating tanh-product form, bit for bit the oracle's ORC_SPA_TANH, 3: the exact rule with every message clipped to LDPC_SPA_CAP (same kernels as 1, LdpcKParams::spa_cap)
    int fast_deg = 0;             // slots per layer in the unrolled kernel (11, 13 or 27)
    bool fast_pad = false;        // layers padded with NULL slots (irregular code)
    int fast_inf_row = -1;        // byte offset of the +inf row the NULL slots read, or -1
    int fast_mode = 0;            // posterior image -- 0: in LDS, 1: in the workgroup's global slot, 3: static hybrid (k_ldpc.hip plan), 4 / 5: static hybrid + 32 / 39 rows parked in the idle waves' registers
    std::vector<uint32_t> nat_tab, nat_haz;   // k_ldpc_nat.hip: natural-row-order tables
    uint32_t *d_nat_tab = nullptr, *d_nat_haz = nullptr;
    bool fast_cu1 = false;        // mode 6: one frame per CU, the whole image on chip (k_ldpc_cu1.hip); fast_wg8 is set too (same tables)
    int cu1_pairs = 0;            // mode 6: pairs of rows that share an LDS position and a register slot of the row-keeping waves
    bool fast_wg8 = false;        // one frame per 8-wave workgroup, SIMD-aware roles, two independent workgroups per CU (k_ldpc_wg8.hip)
    bool w8_dups_in_lds = false;  // static hybrid: every bit-group with two edges in one layer is LDS-resident
    std::vector<uint32_t> w8_tab, w8_rows;
    uint32_t *d_w8_tab = nullptr, *d_w8_rows = nullptr;
    // (round 4) per-lane address table of the min-sum layer: [q][ceil(deg / 4)][LDPC_AT_LANES][4] dwords -- for slot j of layer r and check t the LDS byte address of the
    // posterior (LDS slot) or its rotated byte offset inside the row (global slot): what the layer loop formed with 3-4 vector instructions per slot and iteration
    std::vector<uint32_t> w8_atab;
    uint32_t *d_w8_atab = nullptr;
    uint32_t w8_st_base = 0, w8_lds_junk = 0;
    int w8_lds_bytes = 0, w8_gwork_words = 0, w8_nl_info = 0, w8_nl = 0, w8_ng_info = 0, w8_ng = 0;
    int w8_park_moves = 0;        // mode 4: row moves between LDS and the idle waves' registers per iteration
    uint32_t *d_cu_ctr = nullptr; // [LDPC_CU_CTR_WORDS]
};
constexpr int LDPC_PROF_WORDS = 1024 * 64;   // development aid (LDPC_PHASE_PROF builds): per-wave phase timers
constexpr int LDPC_CU_CTR_WORDS = 4096 + 64;   // [0, 4096): arrivals per CU, key = XCC_ID << 8 | SE_ID << 5 | SH_ID << 4 | CU_ID; [4096]: frames handed out (work queue)
constexpr int LDPC_FRAME_CTR = 4096;
// The min-sum layer's per-lane address table is built and uploaded for the LDS-only image alone (for the LDS slots of the hybrid images too: measured and left off,
// docs/negative_results.md; 0.9-6 MB per handle that no normal-frame kernel reads).
// Sum-product layer, LDS-only image: the slots' LDS addresses from a per-lane table of 16-bit entries (k_ldpc.hip emit_atab_spa16, k_ldpc_wg8.hip AT16) ...
#ifndef LDPC_SPA_AT16_MAXDEG
#define LDPC_SPA_AT16_MAXDEG 13      // ... for the 11- and 13-slot codes only (QPSK-S 3/5: 14.33 -> 13.47 ms per 16384 frames).  The 27-slot layer runs at the 128-register budget of two workgroups
#endif                               // per CU: the 14 registers that carry the table do not exist there (23 / 19 / 8 spilled registers with suffix values every 3rd / 4th / 6th slot: QPSK-S 8/9
                                     // 9.63 -> 13.0 / 11.9 / 11.2 ms, docs/negative_results.md)
constexpr int LDPC_AT_LANES = 384;      // lanes per row of the address table (6 waves; lanes 360 .. 383 hold the junk row / an offset that is dropped)
// LDPC_FAST_STRIDE, LDPC_TANH_ORDER and every other number of the fast kernels' tables: ldpc_layer_table.h
constexpr float LDPC_SPA_CAP = 16.6355324f;      // 2 atanh(1 - FLT_EPSILON): where the messages of AFF3CT's tanh-product rule stop (spa_rule 2 by construction, 3 by a clip)
constexpr int LDPC_FAST_MAXC = 16;
// modes 4 / 5 (k_ldpc_wg8.hip): bit-group rows parked in the registers of a workgroup's two idle waves (3 VGPRs per row and lane) and LDS slots per
// layer (the static hybrid without parked rows, mode 3, has 9).  Mode 5 (min-sum kernel only: the sum-product kernel has no registers for it) parks 39.
__host__ __device__ __forceinline__ constexpr int ldpc_park_nr(int mode) { return mode == 5 ? 39 : 32; }
__host__ __device__ __forceinline__ constexpr int ldpc_park_nl(int mode) { return mode == 5 ? 15 : 14; }
// k_ldpc_wg8.hip: duplicate edges (the slots whose stores are redirected to the junk row) sit in the first ldpc_w8_kd(deg) slots of a layer; from
// there on a slot's store goes where its load came from (one address per LDS slot instead of two).  The padded 13-slot form (32APSK-S 3/4: checks of degree
// 9 .. 13) has its NULL slots there too (at most 4 + 2 duplicates).
__host__ __device__ __forceinline__ constexpr int ldpc_w8_kd(int deg) { return deg == 27 ? 6 : deg == 11 ? 3 : deg == 13 ? 6 : deg; }
// mode 6 (k_ldpc_cu1.hip): one frame per 16-wave workgroup = per CU.  Two lanes per check: the first half-check's lanes take slots 0 .. LDPC_CU1_HA-1 (the duplicate
// edges are among them), the second one's the rest (p_c and p_{c-1} last); they exchange {min1 | parity, min2} through 8 bytes per half-check of LDS.  Four
// row-keeping waves in two groups of two, ldpc_cu1_nrg() rows (3 VGPRs per row and lane) each.
#ifndef LDPC_CU1_HA_V
#define LDPC_CU1_HA_V 14
#endif
constexpr int LDPC_CU1_HA = LDPC_CU1_HA_V;
constexpr int LDPC_CU1_XCHG_BYTES = 2 * LDPC_Z * 8;
__host__ __device__ __forceinline__ constexpr int ldpc_cu1_nrg() { return 36; }
#ifndef LDPC_CU1_DEFAULT
#define LDPC_CU1_DEFAULT 0
#endif
#ifndef LDPC_CU1_SPA_DEFAULT      // the sum-product decoder on normal frames: mode 6 (one frame per CU, two lanes per check, messages inside the Infinity Cache) as the default
#define LDPC_CU1_SPA_DEFAULT 1
#endif
constexpr int LDPC_W8_MISC_BYTES = 96;  // k_ldpc_wg8.hip: words behind the image -- [0..7] SIMD of wave w, [8] first / second workgroup of the CU, [9] next frame, [10..12] vote words, [16..21] BCH remainder of the frame
constexpr int LDPC_SYN_RED = 640;       // entries x^k mod g(x), k = 0 .. 639, of the BCH verification's reduction table (k <= 64 * 5 + 32 * 8 + 63)
constexpr int LDPC_SPA_MAXC = 6;       // SPA: duplicate edges per layer whose old messages a lane keeps in registers (the DVB-S2 codes have at most 6)
constexpr int NAT_AHEAD = 24;           // k_ldpc_nat.hip, lanes-per-frame form: checks whose loads are in flight ahead of the one being computed (8 lanes per frame; 12 with 4 lanes per frame)
constexpr int NAT_HAZ_WINDOW = NAT_AHEAD + 1;
size_t ldpc_nat_group_words(const LdpcPlan &pl);
hipError_t ldpc_wg8_launch(const LdpcPlan &pl, LdpcKParams p, hipStream_t s);
int ldpc_wg8_blocks_per_cu(const LdpcPlan &pl);      // (choosing and launching a call's kernel: ldpc_dispatch.h)

// builds the layer tables; returns empty string on success, else the error text
std::string ldpc_build_plan(LdpcPlan &pl, int N, int K, int n_rows, const int32_t *row_ptr,
                            const int32_t *addr, int lds_groups_req, size_t lds_limit_bytes, int spa_rule = 0, bool small_batch = false);      // small_batch: the handle never sees more frames than CUs      // spa_rule: LdpcPlan::spa_rule

// ---------------------------------------------------------------- BCH (a2)
struct BchPlan {
    int m = 0, n = 0, t = 0, N = 0, K = 0;
    std::vector<uint16_t> exp_, log_;
    uint16_t *d_exp = nullptr, *d_log = nullptr;   // exp has 2n entries (no modulo on sums)
    uint32_t *d_prbs = nullptr;                    // BB scrambler sequence, packed, K bits
    uint32_t *d_prbs_rw = nullptr;                 // the same by (bit-group row, wave) for the LDPC kernel's fused output (LdpcKParams::info_prbs)
    // syndrome tables, one set per odd j = 1, 3, .., 2t-1 (see k_bch.hip):
    //   [0 .. 256)            bit-reversed byte
    //   [256 + 768 k ..)      for the k-th odd j: 256 x (u(x) x^m mod m_j(x)) | 256 x eval(low byte) | 256 x eval(high byte)
    std::vector<uint16_t> syn_tab;
    uint16_t *d_syn_tab = nullptr;
};
struct BchKParams {
    const int32_t *in_bits;     // [F][N] or null
    const uint32_t *in_packed;  // [F][ceil(N/32)] or null
    // (round 5) fused chain behind an LDPC kernel that has verified the frames itself: only frames with flag[f] != 0 are decoded; their first K bits are
    // out_bits (descrambled by the producer: re-scrambled here with `prbs`), the N - K parity bits come from in_packed
    const uint8_t *flag;        // [F] or null (every frame is decoded)
    int32_t *out_bits;          // [F][K]
    int8_t *cwd;                // [F] or null
    const uint16_t *exp_, *log_, *syn_tab;
    const uint32_t *prbs;       // packed K-bit BB descrambling sequence or null (no descramble)
    int32_t patch_only;         // out_bits already holds the (descrambled) uncorrected bits: only flip what the decoder corrects
    int32_t N, K, m, n, t, n_frames;
};
std::string bch_build_plan(BchPlan &pl, int m, const int32_t *prim, int t, int N, int K);
hipError_t bch_launch(const BchPlan &pl, BchKParams p, int grid_cap, hipStream_t s);      // grid_cap: bch_grid() (rx_dispatch.h)

// ---------------------------------------------------------------- front end (a3, a4, a6, a7)
struct FrontKParams {
    const float *in;        // pl frames [F][2*pl_frame] or xfec frames [F][2*n_sym]
    const float *const *src;   // (round 5) per-frame start of the PL frame (8-byte aligned) instead of in + f * 2 * pl_frame: the located form of the frame synchronizer; or null
    const float *sigma_in;  // [F] or null
    float *llr;             // [F][N_ldpc]
    float *est;             // [F][3] sigma, ebn0, esn0 (may be null)
    const float *cstl;      // normalised constellation, 2^bps points
    const uint8_t *pl_seq;  // PL scrambling sequence R(i), 66420 entries
    int32_t n_sym, pl_frame, bps, itl_cols, itl_order, n_frames;
    int32_t slice_chunk;    // front_kernel: symbols per workgroup when a frame is dealt to several (blockIdx.y), 0 = the whole frame (set by the launcher: small batches)
    float code_rate;
    // separable 2-bit constellation (plan time): L_b = c (y[sep_ax[b]] * sep_g[b] + sep_h[b]); sep = 0: general demapper
    int32_t sep, sep_ax[2];
    float sep_g[2], sep_h[2];
};
hipError_t frame_order_launch(const float *llr, float *metric, uint32_t *order, int F, int N, hipStream_t s);      // k_ldpc_generic.hip: the work queue's order for launches with the stopping rule (noisiest frames first)
// a7+a6+a3+a4 fused (in = pl frames) or a3 (+a4) (in = xfec frames, sigma_in required), in the form front_choose chose (rx_dispatch.h)
hipError_t front_launch(FrontKParams p, const FrontChoice &ch, hipStream_t s);
hipError_t deinterleave_launch(const float *itl, float *nat, int N, int cols, int order, int F, hipStream_t s);
hipError_t estimate_launch(const float *x, float *sig, float *ebn0, float *esn0, int n_sym, float code_rate,
                           int bps, int F, hipStream_t s);
hipError_t pl_descramble_launch(const float *in, float *out, const uint8_t *seq, int pl_frame, int F, hipStream_t s);
hipError_t agc_launch(const float *X, float *Z, int n_cplx, float output_energy, int F, hipStream_t s);      // k_agc.hip
hipError_t nco_launch(const float *X, float *Z, float omega, uint32_t n0, long long total, float *FRQ, float *PHS, float frq, int F, hipStream_t s);    // k_agc.hip
hipError_t remove_plh_launch(const float *in, float *out, int n_sym, int pl_frame, int F, hipStream_t s);
hipError_t bb_descramble_launch(const int32_t *in, int32_t *out, const uint32_t *prbs, int K, int F, hipStream_t s);
hipError_t monitor_launch(const int32_t *U, const int32_t *V, unsigned long long *ctr, int K, int F, hipStream_t s);
hipError_t monitor2_launch(const int32_t *U, const int32_t *V, unsigned long long *ctr, int32_t *be_tmp, long long *FRA, int32_t *BE, int32_t *FE, float *BER,
                           float *FER, int K, int F, hipStream_t s);

// ---------------------------------------------------------------- TX mirror + AWGN (N1)
struct TxKParams {
    const int32_t *info_in;     // [F][K_bch] or null: random payload from (seed, frame)
    int32_t *info_out;          // [F][K_bch] or null
    const float *sigma;         // [F] or null: no noise
    float *pl_out;              // [F][2*pl_frame]
    uint32_t *bch_cw;           // [F][ceil(K_ldpc/32)] work
    uint32_t *ldpc_cw;          // [F][ceil(N_ldpc/32)] work
    const uint32_t *prbs;       // BB scrambling sequence, packed
    const uint32_t *enc_tab;    // [q][enc_stride]: t0 | group << 9
    const int32_t *enc_deg;     // [q]
    const float *cstl;          // normalised constellation
    const float *plh;           // 180 floats: PLHEADER
    const uint8_t *pl_seq;
    const unsigned long long *bch_tab;  // [256][3]: (u(x) x^r) mod g(x), byte-wise systematic encoder
    const unsigned long long *bch_shift;   // [16 segments][r][3]: x^(b + 8 * bytes behind the segment) mod g (segmented division)
    uint32_t seed_lo, seed_hi;
    int32_t K_bch, K_ldpc, N_ldpc, bps, itl_cols, itl_order, n_sym, pl_frame, enc_stride, n_frames;
};
hipError_t tx_launch(const TxKParams &p, hipStream_t s);
// the TX tasks at the task boundary (k_tx_tasks.hip): int32 per bit, float pairs per symbol; the encoders take the tables and the B_TXBCH scratch (bch_cw) from p
hipError_t tx_bch_encode_launch(const TxKParams &p, const int32_t *U_K, int32_t *X_N, hipStream_t s);
hipError_t tx_ldpc_encode_launch(const TxKParams &p, const int32_t *U_K, int32_t *X_N, hipStream_t s);
hipError_t tx_interleave_launch(const int32_t *nat, int32_t *itl, int N, int cols, int order, int F, hipStream_t s);
hipError_t tx_modulate_launch(const int32_t *X, float *Y, const float *cstl, int bps, int N, int n_sym, int F, hipStream_t s);
hipError_t tx_framer_launch(const float *X, float *Y, const float *plh, int n_sym, int pl_frame, int F, hipStream_t s);
hipError_t tx_pl_scramble_launch(const float *X, float *Y, const uint8_t *seq, int pl_frame, int F, hipStream_t s);
// generator polynomial of the t-error-correcting BCH code over GF(2^m): g[i] = coeff of x^i
std::vector<uint8_t> bch_generator(const BchPlan &pl);

// ---------------------------------------------------------------- FIR (a5)
// S >= 1 streams of n_per samples per call (dvbs2hip_set_streams), stream s at x + 2 s n_per; the memories of T - 1 samples side by side in hist_in / hist_out.
// ch: fir_choose / upfir_choose (rx_dispatch.h)
hipError_t fir_launch(const float *x, float *y, const float *hist_in, float *hist_out, const float *taps_rev, const uint16_t *afrag, int T, long long n_per, int S, const FirChoice &ch,
                      hipStream_t s);
hipError_t upfir_launch(const float *x, float *y, const float *hist_in, float *hist_out, const float *taps, const uint16_t *afrag2, int T, int osf, long long n_in, const FirChoice &ch,
                        hipStream_t s);
// matrix-core form (k_fir_mfma.hip): bf16 x 3 split operands, fp32 accumulation
std::vector<uint16_t> fir_mfma_afrag(const float *taps_rev, int T);
std::vector<uint16_t> upfir_mfma_afrag(const float *taps, int T);
hipError_t fir_mfma_launch(const float *x, float *y, const float *hist_in, float *hist_out, const uint16_t *afrag, int T, long long n, const FirChoice &ch, hipStream_t s);
hipError_t decimate_launch(const float *x, float *y, long long n_out, int osf, long long offset, long long n_in, hipStream_t s);
hipError_t awgn_launch(const float *x, float *y, const float *sigma, unsigned long long seed, long long n_pairs, int F, hipStream_t s);

// ---------------------------------------------------------------- frame synchronizer (N4, k_sync.hip)
// per-frame results of the frame synchronizer's arg max (sync_finalize_kernel): the sockets, the delay line's table, the handle's state
struct SyncTail {
    unsigned long long *keys;        // F x ceil(n / 64) words of device scratch
    int32_t *delay; float *metric; int32_t *flag; float trigger;
    int32_t *Dtab; float *last_metric;
    float *seg;                      // 2 x ceil(max_frames / SYNC_SUB) x n floats of device scratch: per sub-segment of the call's frames {alpha^len, its own average from 0} (k_sync.hip)
};
// (SYNC_MAX_SEG, SYNC_SUB, SyncSegPlan and sync_segment_plan: rx_dispatch.h)
// S >= 1 streams per call (dvbs2hip_set_streams): Fs = F / S frames per stream, n_per = n Fs samples; xh / sofh (64 complex), cv (n), yprev (2 n), buff2 (nbuff2), st
// (SYNC_ST_STRIDE ints) and last_metric (1) hold the streams side by side, SyncTail's per-frame arrays and keys are stream-major like the sockets
constexpr int SYNC_ST_STRIDE = 4;
// ch: what sync_choose / lr_choose / rotate_choose (rx_dispatch.h) chose for the call
hipError_t sync_corr_launch(const float *x, const float *xh_in, float *xh_out, const uint16_t *frag, float *cor_sof, float *cor_plsc, long long n_per, int S, const SyncChoice &ch,
                            hipStream_t s);
std::vector<uint16_t> sync_mfma_frag(const float *sof25, const float *plsc64);       // k_sync_mfma.hip: band fragments of the two correlators
// corr != null: the one-task form (sofh_in / sofh_out its memories), else both correlations go to their sockets
hipError_t sync_corr_mfma_launch(const float *x, const float *xh_in, float *xh_out, const uint16_t *frag, const float *sofh_in, float *sofh_out, float *corr,
                                 float *cor_sof, float *cor_plsc, long long n_per, int S, unsigned grid, hipStream_t s);
std::vector<uint16_t> sync_frag_default();                                            // k_sync.hip: the fragments of conj_SOF / conj_PLSC
hipError_t sync_corr_metric_launch(const float *x, const float *xh_in, float *xh_out, const uint16_t *frag, const float *sofh_in, float *sofh_out, float *cv, float *corr,
                                   const SyncTail &t, int n, int Fs, int S, float alpha, int vec_width, const SyncChoice &ch, hipStream_t s);
hipError_t sync_metric_launch(const float *cor_sof, const float *sofh_in, float *sofh_out, const float *cor_plsc, float *cv, float *corr,
                              const SyncTail &t, int n, int Fs, int S, float alpha, int vec_width, const SyncChoice &ch, hipStream_t s);
// list / src: the located form (S == 1 only)
hipError_t sync_vdelay_launch(const float *X, const float *Yprev, float *Yprev_new, float *Y, const float *buff_old, float *buff_new, const int *st_old, int *st_new,
                              const int32_t *Dtab, int n, int nbuff2, int Fs, int S, const SyncChoice &ch, hipStream_t s, int32_t *list = nullptr, const float **src = nullptr);
// one launch (recurrence and rotation, err_dev its error word) or three (err_dev unused)
hipError_t sff_lr_launch(const float *X, float *Y, float *R_l, float *tmp, float *FRQ, float *PHS, int n, int F, int S, float alpha, uint32_t *err_dev, const LrChoice &ch, hipStream_t s);
hipError_t sff_lr_recover(const float *X, float *Y, float *tmp, int n, int F, bool pair, hipStream_t s);
hipError_t sff_fp_launch(const float *X, float *Y, float *tmp, float *FRQ, float *PHS, int n, int F, bool pair, hipStream_t s);
// k_pls.hip: the PLHEADER of frame f, at X + 2 f stride_cplx floats or at SRC[f] (8-byte aligned), decoded to V = b0 128 + .. + b6 2 + p; MET, ENE may be null
hipError_t pls_decode_launch(const float *X, const float *const *SRC, size_t stride_cplx, int32_t *PLS, float *MET, float *ENE, int F, hipStream_t s);
// k_pls_search.hip: the same decoder at every symbol offset k of X (n_sym complex symbols, 8-byte aligned), K = n_sym - 89 outputs, bit for bit what pls_decode_launch
// gives for a frame at X + 2 k; MET, ENE may be null.  Then the search of include/dvbs2hip.h on such outputs: LEN int32[256], work pls_search_work_bytes(n_sym) bytes,
// RES int32[4], SCORE one float; two launches
hipError_t pls_scan_launch(const float *X, int n_sym, int32_t *PLS, float *MET, float *ENE, hipStream_t s);
size_t pls_search_work_bytes(int n_sym);
hipError_t pls_search_launch(const int32_t *PLS, const float *MET, const float *ENE, const int32_t *LEN, void *work, int n_sym, int32_t *RES, float *SCORE, hipStream_t s);
// k_pls_walk.hip: the walk of include/dvbs2hip.h over the M candidates start + 18 i whose (PLS, MET, ENE) the caller has put at the head of work (M entries each);
// K = pls_walk_levels(M, the smallest hop LEN allows in candidates, max_out) levels of jumps, work pls_walk_work_bytes(M, K) bytes; lane: one lane follows the chain
// instead (3 + 2 K launches against 2).  LEN int32[256]; SRC may be null
int pls_walk_levels(int M, int min_hop, int max_out);
size_t pls_walk_work_bytes(int M, int K);
hipError_t pls_walk_launch(const float *X, int n_sym, int start, int M, int K, bool lane, const int32_t *LEN, float q_min, int max_out, void *work, int32_t *OFF, int32_t *VAL,
                           float *Q, const float **SRC, int32_t *IDX, int32_t *CNT, int32_t *RES, hipStream_t s);
// k_est_pilots.hip: the pilot-aided noise estimate of frame f, at X + 2 f stride_cplx floats or at SRC[f] (8-byte aligned), from its L = 90 + 36 N_pilots known symbols
// (compact: the frame holds those L symbols and nothing else); plh: the 90 header symbols, seq: the PL sequence (read for scrambled = 1).  AN null: SIG / EB / ES (each
// may be null) are written; AN given: (A, N) per frame and nothing else, and est_pilots_walk_launch averages them per stream (state: 3 floats per stream) and writes the outputs
hipError_t est_pilots_launch(const float *X, const float *const *SRC, size_t stride_cplx, int compact, const float *plh, const uint8_t *seq, int scrambled, int L,
                             float code_rate, int bps, float *AN, float *SIG, float *EB, float *ES, int F, hipStream_t s);
hipError_t est_pilots_walk_launch(const float *AN, float *state, float alpha, int L, float code_rate, int bps, float *SIG, float *EB, float *ES, int Fs, int S, hipStream_t s);

// ---------------------------------------------------------------- BBFRAME layer (k_bbframe.hip)
struct BbfParams {
    int32_t K;               // K_bch
    int32_t uplb;            // user packet length in bytes
    int32_t sync;            // the packets' sync byte
    int32_t matype;          // MATYPE-1 << 8 | MATYPE-2
    int32_t mark_tei;        // a transport packet with a wrong CRC-8 gets its transport_error_indicator set
};
// the states between calls, all zero = reset.  Transmitter, four int32: {pos, the CRC-8 running over the current packet, the CRC-8 of the last complete packet, 0}.
// Receiver: four int32 {have, bytes of the pending packet, 0, 0}, then the pending packet's bytes
constexpr int BBF_TX_STATE = 16, BBF_RX_HEAD = 16;
// U: F frames of K int32 bits (16-byte aligned) from the next n_bytes bytes of the packet stream, (F - 1) D < n_bytes <= F D with D = (K - 80) / 8
hipError_t bbframe_build_launch(const uint8_t *UP, long long n_bytes, int32_t *U, const int32_t *st_in, int32_t *st_out, const BbfParams &p, int F, hipStream_t s);
// V: F descrambled frames (16-byte aligned); VALID, HDR may be null; hdr: 8 F int32 and plan: 4 F int32 of workspace (16-byte aligned); UP, STATUS: room for `cap` packets;
// ctr: the five counters of dvbs2hip_bbframe_get_stats.  Three launches
hipError_t bbframe_parse_launch(const int32_t *V, const int8_t *VALID, int32_t *hdr, int32_t *HDR, int32_t *plan, const uint8_t *st_in, uint8_t *st_out, uint8_t *UP,
                                uint8_t *STATUS, int32_t *N_OUT, unsigned long long *ctr, const BbfParams &p, int cap, int F, hipStream_t s);

// ---------------------------------------------------------------- symbol-timing recovery and the channel's delay tasks (k_timing.hip)
// one stream's state of Synchronizer_Gardner_fast_osf2 between calls (all zeros = _reset): the Farrow history x[n-1], x[n-2], x[n-3], the TED buffer {T0, T1}, mu (the Farrow
// taps follow from it), the NCO, the loop filter, the last symbol, the strobe flags
struct StmState {
    float h[6];
    float ted[4];
    float mu, nco, lf_prev_in, lf_output;
    float last[2];
    int32_t is_strobe, prev_is_strobe;
};
hipError_t stm_sync_launch(const float *X, float *Y, int32_t *B, float *MU, const StmState *st_in, StmState *st_out, int S, int Fs, int N, float kp, float ki, hipStream_t s);
// the held loop (k_timing_ultra.hip): the same state, a wave per stream; H the hold size, act as Synchronizer_timing::set_act
hipError_t stm_ultra_launch(const float *X, float *Y, int32_t *B, float *MU, const StmState *st_in, StmState *st_out, int S, int Fs, int N, int H, int act, float kp, float ki,
                            hipStream_t s);
hipError_t stm_extract_launch(const float *Y1, const int32_t *B1, float *Y2, int32_t *UFW, int32_t *RDY, const float *c_in, const int32_t *n_in, float *c_out, int32_t *n_out,
                              int32_t *uf, int S, int Fs, int N, long long cap, hipStream_t s);
hipError_t chn_delay_launch(const float *X, float *Y, const float *h_in, float *h_out, long long H, long long T, float b0, float b1, float b2, hipStream_t s);

// ---------------------------------------------------------------- the coarse-frequency loop (k_stepmf.hip)
// one stream's state of Synchronizer_freq_coarse_DVBS2_aib and its Multiplier_sine_ccc_naive between calls, and Synchronizer_step_mf_cc::last_delay: the detector's two
// previous pilot symbols, the PI filter, the integrator, estimated_freq, nu in millionths of a cycle per sample (set_nu floors it to six decimals), the sample counter
// n = 0 .. 999999, the symbol index in the frame.  _reset: all zero but curr_idx = pl_frame - 1; last_delay survives it (Synchronizer_step_mf_cc::reset does not touch it)
struct SfcState {
    float prev[2], pprev[2];
    float lfs, ifs, dds;
    float est;
    int32_t nu_k, n, curr_idx, last_delay;
};
hipError_t stepmf_launch(const float *X, float *Y, int32_t *B, float *MU, float *FRQ, float *PHS, const int32_t *DEL, const int32_t *ccnt, const StmState *st_in, StmState *st_out,
                         const SfcState *cf_in, SfcState *cf_out, const float *hist_in, float *hist_out, const float *taps, const float *P, int n_p, int S, int Fs, int N, int pl_frame,
                         float kp, float ki, float pg, float ig, float sps, hipStream_t s);
// the same loop and the same state, a wave per stream (k_stepmf_wave.hip): rotation and matched filter of 64 samples ahead of the serial steps
hipError_t stepmf_wave_launch(const float *X, float *Y, int32_t *B, float *MU, float *FRQ, float *PHS, const int32_t *DEL, const int32_t *ccnt, const StmState *st_in,
                              StmState *st_out, const SfcState *cf_in, SfcState *cf_out, const float *hist_in, float *hist_out, const float *taps, const float *P, int n_p, int S,
                              int Fs, int N, int pl_frame, float kp, float ki, float pg, float ig, float sps, hipStream_t s);

}  // namespace dvbs2
