// Which LDPC kernel decodes a call: ONE description (LdpcChoice), ONE function that makes it (ldpc_choose: host arithmetic on the plan and the call's facts, no handle, no
// device) and ONE that launches it (ldpc_launch).  What the handle's other code wants to know about the kernel of a call -- its name, whether it writes the chain's output
// socket, whether it verifies the BCH remainder, whether it takes a frame order, how many of its workgroups a CU holds -- is read from the choice and derived nowhere else.
#pragma once
#include "dvbs2hip_internal.h"

namespace dvbs2 {

enum LdpcFamily { LF_GENERIC, LF_WG8, LF_CU1, LF_LAT, LF_NAT_LANE, LF_NAT_PART, LF_NAT_CK, LF_NAT_SPA, LF_COUNT };

struct LdpcCallFacts {
    int schedule;          // DVBS2HIP_SCHED_QC / DVBS2HIP_SCHED_NATURAL
    int F;                 // frames of the call (INT32_MAX: the kernel of a batch too large for any small-batch form -- what the handle sizes its persistent grid and builds its tables for)
    int n_cus;
    bool lat_lds_ok;       // a workgroup may own 160 KiB of LDS
    bool early_stop;
    bool syn_tables;       // the BCH-verification tables of the fused chain exist (LdpcKParams::syn_tab)
};

struct LdpcChoice {
    LdpcFamily family = LF_GENERIC;
    int targ[3] = {0, 0, 0};      // the instantiation's template arguments in the kernel's order (bool as 0 / 1; unused ones 0)
    bool writes_info = false;     // the kernel fills LdpcKParams::info_out
    bool writes_bch = false;      // ... and bch_flag / cwd_bch
    bool takes_order = false;     // ... and hands its frames out in LdpcKParams::order
    int block = 0;                // threads per workgroup
    size_t lds_bytes = 0;         // dynamic LDS per workgroup
    int blocks_per_cu = 0;        // resident workgroups per CU by design (wg8: at most; 0: whatever fits -- the runtime's answer is ldpc_blocks_per_cu)
    std::string error;            // not empty: the plan asks for an instantiation that does not exist; nothing is launched
};

constexpr int LDPC_WG8_THREADS = 512, LDPC_CU1_THREADS = 1024, LDPC_LAT_THREADS = 768, LDPC_LAT_ROW = LDPC_Z * 4;      // (asserted against the kernels' own constants in their files)

LdpcChoice ldpc_choose(const LdpcPlan &pl, const LdpcCallFacts &c);
struct LdpcFamilyInfo { const char *kernel; int n_targ; };      // the family's __global__ function and how many template arguments it has
const LdpcFamilyInfo &ldpc_family(LdpcFamily f);
bool ldpc_has(LdpcFamily family, const int *targ);                       // this instantiation is built
std::string ldpc_choice_name(const LdpcChoice &ch);        // what dvbs2hip_ldpc_kernel_name says
hipError_t ldpc_launch(const LdpcPlan &pl, const LdpcChoice &ch, LdpcKParams p, float *nat_work, hipStream_t s);      // nat_work: the natural order's workspace (else unused)
int ldpc_blocks_per_cu(const LdpcPlan &pl, const LdpcChoice &ch);      // asks the device (persistent-grid families)

// the plan-derived fields of LdpcKParams that every QC-layer launcher sets the same way
void ldpc_plan_params(const LdpcPlan &pl, LdpcKParams &p);

// Each family's table of instantiations lives next to its kernels: whether one exists, and the launch (occupancy) of the one a choice names.
// (k_ldpc_wg8.hip keeps its own dispatch; ldpc_dispatch.hip lists its instantiations and checks a plan against the list before calling it.)
bool ldpc_generic_has(const int *targ);
hipError_t ldpc_generic_launch(const LdpcPlan &pl, const LdpcChoice &ch, LdpcKParams p, hipStream_t s);
int ldpc_generic_blocks_per_cu(const LdpcPlan &pl, const LdpcChoice &ch);
bool ldpc_cu1_has(const int *targ);
hipError_t ldpc_cu1_launch(const LdpcPlan &pl, const LdpcChoice &ch, LdpcKParams p, hipStream_t s);
bool ldpc_lat_has(const int *targ);
hipError_t ldpc_lat_launch(const LdpcPlan &pl, const LdpcChoice &ch, LdpcKParams p, hipStream_t s);
bool ldpc_nat_has(LdpcFamily family, const int *targ);
hipError_t ldpc_nat_launch(const LdpcPlan &pl, const LdpcChoice &ch, const LdpcKParams &kp, float *work, hipStream_t s);

// raises KERN's dynamic-LDS limit to `bytes`: one hipFuncSetAttribute per kernel and device (and per larger size)
template <auto KERN>
static hipError_t ldpc_dyn_lds(size_t bytes)
{
    static size_t configured[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (bytes <= configured[dev & 63]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) configured[dev & 63] = bytes;
    return e;
}

}  // namespace dvbs2
