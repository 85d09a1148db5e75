// Which kernel runs a call of the receive path outside the LDPC decoder (that one: ldpc_dispatch.h): ONE function per stage makes the choice from the call's facts as plain
// values -- pointers enter as their alignment only -- and the *_launch functions of the k_*.hip files launch what it says.  Host arithmetic only: no kernel, no handle,
// no HIP call; tools/plan_probe.cpp prints the choices and tests/test_rx_dispatch.py walks them on the CPU.  Every environment variable that steers a choice is read
// inside these functions, at every call, and nowhere else (the list: rx_dispatch.hip).
#pragma once
#include <stdint.h>
#include <string>

namespace dvbs2 {

// bytes a pointer is aligned to, 16 at the most (what the widest access of any kernel here asks for)
inline unsigned ptr_align(const void *p) { const uintptr_t a = reinterpret_cast<uintptr_t>(p) | 16u; return (unsigned)(a & (~a + 1)); }

// ---------------------------------------------------------------- front end (k_front.hip)
constexpr int FRONT_THREADS = 256;      // lanes per workgroup of the two-sweep front_kernel
constexpr int FRONT_WIDE = 1024;        // lanes per frame of the register-resident kernels
// Symbols a lane of front_kernel demaps per trip of its loop (= per read of the constellation table); front_choose cuts a frame into slices of whole trips with the same
// number.  Two per lane for the APSK constellations: 16APSK-N 0.396 against 0.402 ms, 32APSK-S 0.179 against 0.129 (registers).
constexpr int front_syms_per_trip(int bps) { return bps <= 3 ? 4 : 1; }

enum FrontForm { FRONT_REG2, FRONT_REG, FRONT_TWO_SWEEP };
struct FrontFacts {
    int bps; bool sep;                   // bits per symbol; the mapping is marked separable (FrontKParams::sep)
    int itl_cols, n_sym, pl_frame, F;
    unsigned align_pl, align_llr;        // ptr_align of the PL socket (ignored for a located call: its frames come through a buffer descriptor) and of the LLR socket
    bool located, from_pl, deinterleave; // from_pl: the fused front end on PL frames; else the demapper on XFEC frames, with or without the de-interleaver
};
struct FrontChoice {
    FrontForm form = FRONT_TWO_SWEEP;
    int targ[3] = {0, 0, 0};             // FRONT_REG2: <PPT>; FRONT_REG: <BPS, SPT, SEP>; FRONT_TWO_SWEEP: <BPS, FROM_PL, DEITL>
    int block = FRONT_THREADS;
    int grid_y = 1, slice_chunk = 0;     // FRONT_TWO_SWEEP: workgroups per frame and the symbols each takes (0: the whole frame)
    bool error = false;                  // no instantiation for this bps; nothing is launched
};
FrontChoice front_choose(const FrontFacts &c);
std::string front_choice_name(const FrontChoice &ch);      // `front_reg_kernel<3, 22, false>`, `front_kernel<5, true, true> sliced`

// ---------------------------------------------------------------- FIR (k_fir.hip, k_fir_mfma.hip)
constexpr int FIR_THREADS = 256;
constexpr int FIR_R = 8;                          // outputs per lane
constexpr int FIR_TILE = FIR_THREADS * FIR_R;     // outputs per workgroup
constexpr int FIR_TMAX = 257;
constexpr int UP_THREADS = 256;
constexpr int FM_TILE = 2048;                     // outputs per workgroup = 8 MFMA tiles of 256
constexpr int FM_H = 80;                          // history the Toeplitz band is laid out for (T = 81)

enum FirFamily { FIR_MFMA, FIR_VECTOR };
struct FirChoice {
    FirFamily family = FIR_VECTOR;
    int taps = 0;                        // FIR_VECTOR, matched filter: the compile-time tap count (81) or 0 = run-time T
    bool streams = false;                // the S > 1 instantiation, one grid row per stream
    bool up = false;                     // the up-sampling filter (FIR_MFMA: its two branches over the same staged samples)
    int tiles_per_wg = 1;                // FIR_MFMA
    unsigned grid_x = 0, grid_y = 1;
    bool error = false;                  // T, S, osf or the length out of range
};
// have_frag: the band fragments exist and the handle has not been told to keep the vector kernel (dvbs2hip_set_filter_kernel)
FirChoice fir_choose(int T, long long n_per, int S, unsigned align_x, unsigned align_y, bool have_frag);
FirChoice upfir_choose(int T, int osf, long long n_in, unsigned align_x, unsigned align_y, bool have_frag);
std::string fir_choice_name(const FirChoice &ch);

// ---------------------------------------------------------------- frame synchronizer (k_sync.hip, k_sync_mfma.hip)
constexpr int SYNC_MAX_SEG = 8, SYNC_SUB = 64;
constexpr int SYNC_UF96_MAX_WG = 256;      // calls with at most this many workgroups (one per CU) take the thirteen-wave arg max, longer frames the four-wave form of round 3
constexpr int SY_THREADS = 256;
constexpr int SY_R = 4;                       // outputs per lane
constexpr int SY_T = SY_THREADS * SY_R;       // outputs per workgroup of the vector correlators
constexpr int SM_THREADS = 256;
constexpr int SM_TILE = 2048;                 // outputs per workgroup of the matrix-core correlators
constexpr int VD_SPL = 2;                     // PAIRS of complex samples per lane of the delay line, their loads in flight together
// how a one-stream call of F frames of n positions is cut for the average over frames (k_sync.hip): nseg segments of seg_F frames side by side, the last one perhaps shorter;
// nseg = 1 (seg_F = F) is the single walk.  cap: the most segments allowed (DVBS2HIP_SYNC_SEGMENTS, else SYNC_MAX_SEG); have_scratch: SyncTail::seg is there.
// With nseg > 1 seg_F is a multiple of the chunk's 96 frames and of SYNC_SUB, and (nseg - 1) (seg_F / SYNC_SUB) sub-segments take a {A, B} each in the scratch.
// (Frames too long for the thirteen-wave form -- more than 256 workgroups of 64 positions -- are never cut.)
struct SyncSegPlan { int nseg, seg_F; };
SyncSegPlan sync_segment_plan(int n, int F, int cap, bool have_scratch);

enum SyncCorr { SYNC_CORR_MFMA, SYNC_CORR_VALU };
enum SyncArgmax { SYNC_ARGMAX_STREAMS, SYNC_ARGMAX4, SYNC_ARGMAX96 };
struct SyncFacts {
    int n, Fs, S;                        // positions per frame, frames per stream, streams
    int nbuff2;                          // floats of the delay line
    unsigned align_x;
    bool have_frag, have_seg;            // the correlators' band fragments / the segments' scratch (SyncTail::seg) exist
    bool one_task;                       // dvbs2hip_sync_frame_synchronize*: the correlations are no sockets; else synchronize1 + synchronize2
    bool located;
};
struct SyncChoice {
    SyncCorr corr = SYNC_CORR_VALU;
    bool fused = false;                  // one_task: correlators and metric in one launch; false with one_task: the two tasks through device scratch (DVBS2HIP_SYNC_UNFUSED)
    unsigned corr_grid = 0;              // workgroups per stream of the correlators
    SyncArgmax argmax = SYNC_ARGMAX4;
    SyncSegPlan seg = {1, 0};            // SYNC_ARGMAX96
    int nwg = 0;                         // workgroups of 64 positions
    int vd_gx = 0, vd_gy = 0;            // the delay line's grid (its third dimension is S)
};
SyncChoice sync_choose(const SyncFacts &c);
std::string sync_corr_name(const SyncFacts &c, const SyncChoice &ch);      // the kernel that forms the correlations (two tasks) or the metric from the samples (one task)
std::string sync_argmax_name(const SyncChoice &ch);

// ---------------------------------------------------------------- L&R and the rotations (k_sync.hip)
constexpr int SFF_RU = 4, SFF_RCH = 256 * SFF_RU;        // 16-byte pairs per lane / per workgroup of the one-launch form
struct LrChoice {
    bool one_launch = false;             // recurrence and rotation in sff_lr_fused_kernel; else pilots, recurrence, rotation
    unsigned long long timeout_us = 0;   // one_launch: how long a rotating workgroup waits for its estimate
    int cpf = 0;                         // one_launch: workgroups per frame
    bool pair = false;                   // three launches: the rotation as rotate_choose has it
};
bool rotate_choose(int n, unsigned align_x, unsigned align_y);      // true: two samples per lane (sff_rotate2_kernel), false: one (sff_rotate_kernel)
LrChoice lr_choose(int S, int n, unsigned align_x, unsigned align_y);
std::string lr_choice_name(const LrChoice &ch);

// ---------------------------------------------------------------- PLHEADER walk, BCH
constexpr int PLSW_LANE_LEVELS = 5;      // levels up to which one lane follows the chain instead: results/pls_walk/README.md has the measurement
bool pls_walk_choose(int K);             // true: one lane follows the chain, false: K levels of jumps
int bch_grid();                          // the most workgroups of the BCH decoder's persistent grid

}  // namespace dvbs2
