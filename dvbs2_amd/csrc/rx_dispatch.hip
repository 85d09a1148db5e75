// The receive path's choosers (rx_dispatch.h).  No kernel, no handle and no HIP call in this file.
// Every environment variable that steers a choice is read here and nowhere else, at every call:
//   DVBS2HIP_FRONT_TWO_SWEEP  QPSK and 8PSK past the register-resident front end, onto the two-sweep front_kernel
//   DVBS2HIP_FRONT_SINGLE     separable QPSK on the one-symbol-per-access front_reg_kernel instead of the pair kernel
//   DVBS2HIP_FIR=valu         the matched filter on the vector kernel
//   DVBS2HIP_FIR_WGS          caps the matrix-core matched filter's grid (per stream)
//   DVBS2HIP_SYNC=valu        the frame synchronizer's correlators as fp32 vector sums in the reference's order instead of the matrix cores
//   DVBS2HIP_SYNC_UNFUSED     the one-task synchronizer as its two tasks through device scratch (same numbers)
//   DVBS2HIP_SYNC_ARGMAX4     round 3's four-wave arg max for every frame length
//   DVBS2HIP_SYNC_SEGMENTS    the most segments of the average over frames (1 = the single walk)
//   DVBS2HIP_LR=unfused       L&R as three launches
//   DVBS2HIP_LR_TIMEOUT_US    the one-launch L&R's waiting limit (tests: 0 makes every waiting workgroup give up at its first unsuccessful poll)
//   DVBS2HIP_PLS_WALK_FORM    lane | levels: a measurement aid (tools/bench_pls_walk.py times the two forms on one buffer)
//   DVBS2HIP_BCH_GRID         the BCH decoder's persistent grid
#include "rx_dispatch.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace dvbs2 {

static bool env_set(const char *name) { return getenv(name) != nullptr; }
static bool env_is(const char *name, const char *v) { const char *e = getenv(name); return e && !strcmp(e, v); }
static int env_int(const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; }

// ---------------------------------------------------------------- front end
FrontChoice front_choose(const FrontFacts &c)
{
    FrontChoice ch;
    if (c.from_pl && !env_set("DVBS2HIP_FRONT_TWO_SWEEP")) {
        const bool small = c.n_sym <= 8 * FRONT_WIDE, mid = c.n_sym <= 22 * FRONT_WIDE, big = c.n_sym <= 32 * FRONT_WIDE;
        // (a located frame starts on 8 bytes: the pair kernel reads it through a buffer descriptor, which takes any dword address)
        const bool pair_ok = c.bps == 2 && c.sep && c.itl_cols <= 1 && c.n_sym % 2 == 0 && c.pl_frame % 2 == 0 && !env_set("DVBS2HIP_FRONT_SINGLE") &&
                             (c.located || c.align_pl >= 16) && c.align_llr >= 16;
        auto reg = [&](FrontForm form, int a, int b, int s) { ch.form = form; ch.targ[0] = a; ch.targ[1] = b; ch.targ[2] = s; ch.block = FRONT_WIDE; return ch; };
        if (pair_ok && small) return reg(FRONT_REG2, 4, 0, 0);
        if (pair_ok && big) return reg(FRONT_REG2, 16, 0, 0);
        // one symbol per lane and access: short frames (8 symbols per lane) and the 8PSK normal frame (21600 symbols: 22 per lane = 44 registers
        // of frame, which leaves the demapper its own; round 2's 32-per-lane 8PSK form spilled frame symbols and is gone).  A separable QPSK normal frame that
        // cannot take the pair kernel (unaligned sockets) still runs the 32-per-lane QPSK form below (no spills since the estimator's finish lost its powf / log10f);
        // a non-separable mapping goes to the two-sweep kernel
        if (c.bps == 2 && c.sep && small) return reg(FRONT_REG, 2, 8, 1);
        if (c.bps == 2 && c.sep && big) return reg(FRONT_REG, 2, 32, 1);
        if (c.bps == 2 && small) return reg(FRONT_REG, 2, 8, 0);
        if (c.bps == 3 && small) return reg(FRONT_REG, 3, 8, 0);
        if (c.bps == 3 && mid) return reg(FRONT_REG, 3, 22, 0);
        // (round 4: the APSK frames in registers as well -- front_reg_kernel<4, 4>, <4, 16>, <5, 4> -- measured 0.398 against 0.398 ms (16APSK-N), 0.098 against 0.093 (16APSK-S),
        // 0.136 against 0.121 (32APSK-S): with sigma given they read the frame once either way, and the two-sweep kernel overlaps eight workgroups per CU)
    }
    ch.targ[0] = c.bps; ch.targ[1] = c.from_pl; ch.targ[2] = c.from_pl || c.deinterleave;
    ch.error = c.bps < 1 || c.bps > 5;
    if (!ch.error && c.F < 512) {      // fewer workgroups than the chip holds: several per frame
        const int trip = front_syms_per_trip(c.bps) * FRONT_THREADS;      // symbols a workgroup takes per trip of its loop
        const int slices = std::min((c.n_sym + trip - 1) / trip, 1024 / c.F);
        if (slices > 1) { ch.slice_chunk = ((c.n_sym + slices - 1) / slices + trip - 1) / trip * trip; ch.grid_y = (c.n_sym + ch.slice_chunk - 1) / ch.slice_chunk; }
    }
    return ch;
}

std::string front_choice_name(const FrontChoice &ch)
{
    char buf[64];
    const int *t = ch.targ;
    if (ch.error) return "no front_kernel for " + std::to_string(t[0]) + " bits per symbol";
    if (ch.form == FRONT_REG2) snprintf(buf, sizeof buf, "front_reg2_kernel<%d>", t[0]);
    else if (ch.form == FRONT_REG) snprintf(buf, sizeof buf, "front_reg_kernel<%d, %d, %s>", t[0], t[1], t[2] ? "true" : "false");
    else snprintf(buf, sizeof buf, "front_kernel<%d, %s, %s>%s", t[0], t[1] ? "true" : "false", t[2] ? "true" : "false", ch.slice_chunk ? " sliced" : "");
    return buf;
}

// ---------------------------------------------------------------- FIR
// Chunks of 4 tiles, handed to the CUs by the hardware dispatcher as workgroups retire: resident workgroups do not run at
// the same speed (the arbiter favours the older waves), and one persistent workgroup per slot with an equal share of the
// stream waited for the slowest -- same-box sweep at 68 M samples: 1024 workgroups (33 tiles each) 0.222 ms, 8192 (5 tiles)
// 0.207 ms, 16384 0.211 ms.  Short streams still get one workgroup per tile.  max_wg > 0 caps the grid (per stream) instead.
static void fir_mfma_grid(FirChoice &ch, long long n, int max_wg)
{
    const long long n_tiles = (n + FM_TILE - 1) / FM_TILE;
    ch.tiles_per_wg = max_wg > 0 ? (int)((n_tiles + max_wg - 1) / max_wg) : (n_tiles >= 4096 ? 4 : (int)((n_tiles + 1023) / 1024));
    ch.grid_x = (unsigned)((n_tiles + ch.tiles_per_wg - 1) / ch.tiles_per_wg);
}

FirChoice fir_choose(int T, long long n_per, int S, unsigned align_x, unsigned align_y, bool have_frag)
{
    FirChoice ch;
    ch.streams = S > 1; ch.grid_y = (unsigned)S;
    if (T < 1 || T > FIR_TMAX || S < 1 || S > 65535 || n_per < 1) { ch.error = true; return ch; }
    // the matrix-core kernel loads 16 bytes at a time: the sockets have to be so aligned, and with S > 1 streams every stream has to start on such a boundary (n_per even)
    const char *force = getenv("DVBS2HIP_FIR");
    if (have_frag && !(force && force[0] == 'v') && T <= FM_H + 1 && n_per >= 2 && (S == 1 || n_per % 2 == 0) && align_x >= 16 && align_y >= 16) {
        ch.family = FIR_MFMA;
        fir_mfma_grid(ch, n_per, env_int("DVBS2HIP_FIR_WGS", 0));
        return ch;
    }
    ch.taps = T == 81 ? 81 : 0;
    ch.grid_x = (unsigned)((n_per + FIR_TILE - 1) / FIR_TILE);
    return ch;
}

FirChoice upfir_choose(int T, int osf, long long n_in, unsigned align_x, unsigned align_y, bool have_frag)
{
    FirChoice ch;
    ch.up = true;
    if (T < 1 || T > FIR_TMAX || osf < 1 || osf > 16) { ch.error = true; return ch; }
    // osf = 2 and a branch of at most 49 taps: the matrix-core kernel skips the band's first K step
    if (have_frag && osf == 2 && (T - 1) / 2 + 1 <= FM_H + 1 - 32 && n_in >= 2 && align_x >= 16 && align_y >= 16) {
        ch.family = FIR_MFMA;
        fir_mfma_grid(ch, n_in, 0);
        return ch;
    }
    const int per_blk = UP_THREADS / osf;      // input samples per workgroup
    ch.grid_x = (unsigned)((n_in + per_blk - 1) / per_blk);
    return ch;
}

std::string fir_choice_name(const FirChoice &ch)
{
    if (ch.error) return "FIR: a parameter out of range";
    if (ch.family == FIR_MFMA) return "fir_mfma_kernel<" + std::to_string((ch.up ? 2 : 1) + (ch.streams ? 4 : 0)) + ">";
    if (ch.up) return "upfir_kernel";
    return "fir_ccr_kernel<" + std::to_string(ch.taps) + (ch.streams ? ", true>" : ", false>");
}

// ---------------------------------------------------------------- frame synchronizer
// segments of the call's frames side by side while they fit the chip (one workgroup per CU) and stay long enough to be worth a seam (>= 768 frames each)
SyncSegPlan sync_segment_plan(int n, int F, int cap, bool have_scratch)
{
    const int nwg = (n + 63) / 64;
    int nseg = cap <= 1 || !have_scratch ? 1 : std::min(std::min(std::min(cap, SYNC_MAX_SEG), SYNC_UF96_MAX_WG / nwg), F / 768);
    int seg_F = F;
    if (nseg > 1) { seg_F = ((F + nseg - 1) / nseg + 191) / 192 * 192; nseg = (F + seg_F - 1) / seg_F; }      // (a multiple of the chunk's 96 frames and of SYNC_SUB)
    if (nseg <= 1) { nseg = 1; seg_F = F; }
    return {nseg, seg_F};
}

SyncChoice sync_choose(const SyncFacts &c)
{
    SyncChoice ch;
    const long long n_per = (long long)c.n * c.Fs;
    // the matrix-core kernel loads 16 bytes at a time: the socket has to be so aligned, and with S > 1 streams every stream has to start on such a boundary (n_per even)
    ch.corr = c.have_frag && !env_is("DVBS2HIP_SYNC", "valu") && c.align_x >= 16 && (c.S == 1 || n_per % 2 == 0) ? SYNC_CORR_MFMA : SYNC_CORR_VALU;
    ch.corr_grid = ch.corr == SYNC_CORR_MFMA ? (unsigned)((n_per + SM_TILE - 1) / SM_TILE) : (unsigned)((n_per + SY_T - 1) / SY_T);
    ch.fused = c.one_task && (c.located || !env_set("DVBS2HIP_SYNC_UNFUSED"));      // (the located form has no two-task twin)
    ch.nwg = (c.n + 63) / 64;
    // the streams supply the parallelism: the plain walk, one wave per (stream, 64 positions).  One stream, few positions (short frames): the thirteen-wave form, one
    // workgroup per CU at most; long frames: round 3's four-wave form (the stage is bound by its 4 bytes per sample there: QPSK-N 1024 frames 42-45 us in the
    // four-wave form, 65 us in this one)
    if (c.S > 1) ch.argmax = SYNC_ARGMAX_STREAMS;
    else if (!env_set("DVBS2HIP_SYNC_ARGMAX4") && ch.nwg <= SYNC_UF96_MAX_WG) {
        ch.argmax = SYNC_ARGMAX96;
        ch.seg = sync_segment_plan(c.n, c.Fs, env_int("DVBS2HIP_SYNC_SEGMENTS", SYNC_MAX_SEG), c.have_seg);
    }
    const int tot = ((c.nbuff2 > 2 * c.n ? c.nbuff2 : 2 * c.n) + 3) / 4;     // pairs of complex samples
    ch.vd_gx = (tot + 256 * VD_SPL - 1) / (256 * VD_SPL);
    // located: rows of the grid share the list's entries: in lock three of them have work (first frame, last frame, state row), while the synchronizer acquires all do
    ch.vd_gy = c.located && c.Fs + 1 >= 64 ? 64 : c.Fs + 1;
    return ch;
}

std::string sync_corr_name(const SyncFacts &c, const SyncChoice &ch)
{
    const bool one = c.one_task && ch.fused;
    if (ch.corr == SYNC_CORR_MFMA) return std::string(c.S > 1 ? "sync_corr_mfma_streams_kernel<" : "sync_corr_mfma_kernel<") + (one ? "true>" : "false>");
    return std::string(one ? "sync_corr_m_kernel<" : "sync_corr_kernel<") + (c.S > 1 ? "true>" : "false>");
}

std::string sync_argmax_name(const SyncChoice &ch)
{
    return ch.argmax == SYNC_ARGMAX_STREAMS ? "sync_average_argmax_streams_kernel" : ch.argmax == SYNC_ARGMAX4 ? "sync_metric_argmax4_kernel" : "sync_metric_argmax_kernel<96>";
}

// ---------------------------------------------------------------- L&R
// even frame lengths (every DVB-S2 PL frame) and 16-byte aligned sockets: two samples of one frame per lane, 16 bytes per access
bool rotate_choose(int n, unsigned align_x, unsigned align_y) { return n % 2 == 0 && align_x >= 16 && align_y >= 16; }

// S == 1: one launch with its error word, or the three kernels (DVBS2HIP_LR=unfused, an odd frame length, unaligned sockets).  S > 1 streams per call
// (dvbs2hip_set_streams): always the three kernels (the one-launch form's waiting workgroups rely on workgroup 0 being placed first: one assumption per launch, not
// multiplied by the streams)
LrChoice lr_choose(int S, int n, unsigned align_x, unsigned align_y)
{
    LrChoice ch;
    ch.pair = rotate_choose(n, align_x, align_y);
    ch.one_launch = S == 1 && ch.pair && !env_is("DVBS2HIP_LR", "unfused");
    if (ch.one_launch) {
        const char *ev = getenv("DVBS2HIP_LR_TIMEOUT_US");      // one second of wall-clock time unless told otherwise
        ch.timeout_us = ev ? (unsigned long long)atoll(ev) : 1000000ull;
        ch.cpf = (n / 2 + SFF_RCH - 1) / SFF_RCH;
    }
    return ch;
}

std::string lr_choice_name(const LrChoice &ch) { return ch.one_launch ? "sff_lr_fused_kernel" : ch.pair ? "sff_rotate2_kernel<0>" : "sff_rotate_kernel<0>"; }

// ---------------------------------------------------------------- PLHEADER walk, BCH
bool pls_walk_choose(int K)
{
    if (env_is("DVBS2HIP_PLS_WALK_FORM", "lane")) return true;
    if (env_is("DVBS2HIP_PLS_WALK_FORM", "levels")) return false;
    return K <= PLSW_LANE_LEVELS;
}

// about the number of workgroups the chip holds at once
int bch_grid() { return env_int("DVBS2HIP_BCH_GRID", 2048); }

}  // namespace dvbs2
