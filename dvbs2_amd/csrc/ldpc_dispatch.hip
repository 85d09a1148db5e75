// The LDPC launch path's one owner (ldpc_dispatch.h): the kernel of a call is chosen here, from the plan and the call's facts, and launched from here.  No kernel in this file.
// Every environment variable that steers the choice is read in ldpc_choose and nowhere else, at every call:
//   DVBS2HIP_LDPC_LAT=1       small batches of an LDS-only min-sum plan on the two-lanes-per-check kernel (k_ldpc_lat.hip; measured slower, docs/negative_results.md)
//   DVBS2HIP_CHAIN_UNFUSED    the LDPC kernel leaves the chain's output socket to the BCH stage
//   DVBS2HIP_CHAIN_SYN=0      ... writes it, but leaves the BCH remainder to the BCH stage (round 4's form)
//   DVBS2HIP_LDPC_ORDER=1     the work queue hands out the noisiest frames first (k_ldpc_generic.hip: frame_order_launch; measured a loss)
//   DVBS2HIP_NAT_PARTS        the natural order's form: 1 | 4 | 8 lanes per frame, or CK WV = 88 | 44 | 82 | 81 | 41 | 48 checks side by side, waves per workgroup
#include "ldpc_dispatch.h"

namespace dvbs2 {

// ldpc_wg8_kernel<DEG, MODE, SPA> as k_ldpc_wg8.hip instantiates it (its own dispatch ends in an unconditional <27, 1>: a plan is held against this list first)
static bool wg8_has(const int *targ)
{
    const int deg = targ[0], mode = targ[1], rule = targ[2];
    if (rule < 0 || rule > 3) return false;
    if (deg == 11 || deg == 13) return mode == 0 || mode == 1;
    return deg == 27 && (mode == 0 || mode == 1 || mode == 3 || mode == 4 || (mode == 5 && rule == 0));
}

const LdpcFamilyInfo &ldpc_family(LdpcFamily f)
{
    static const LdpcFamilyInfo info[LF_COUNT] = {{"ldpc_layered_nms_kernel", 3}, {"ldpc_wg8_kernel", 3}, {"ldpc_cu1_kernel", 2}, {"ldpc_lat_kernel", 1},
                                                  {"ldpc_nat_kernel", 1}, {"ldpc_nat_part_kernel", 3}, {"ldpc_nat_ck_kernel", 3}, {"ldpc_nat_spa_kernel", 2}};
    return info[f];
}

bool ldpc_has(LdpcFamily family, const int *t)
{
    return family == LF_GENERIC ? ldpc_generic_has(t) : family == LF_WG8 ? wg8_has(t) : family == LF_CU1 ? ldpc_cu1_has(t) : family == LF_LAT ? ldpc_lat_has(t) : ldpc_nat_has(family, t);
}

// the instantiation <t[0], ..> of a family as the call's kernel; one that is not built is the choice's error, never another kernel
static LdpcChoice &pick(LdpcChoice &ch, LdpcFamily family, const int (&t)[3], int block, size_t lds_bytes, int blocks_per_cu)
{
    ch.family = family; ch.block = block; ch.lds_bytes = lds_bytes; ch.blocks_per_cu = blocks_per_cu;
    for (int i = 0; i < 3; i++) ch.targ[i] = t[i];
    if (!ldpc_has(family, t)) {
        ch.error = std::string("LDPC: the plan asks for ") + ldpc_family(family).kernel + "<" + std::to_string(t[0]);
        for (int i = 1; i < ldpc_family(family).n_targ; i++) ch.error += "," + std::to_string(t[i]);
        ch.error += ">, which is not built";
    }
    return ch;
}

LdpcChoice ldpc_choose(const LdpcPlan &pl, const LdpcCallFacts &c)
{
    auto env_is = [](const char *name, char v) { const char *e = getenv(name); return e && e[0] == v; };
    LdpcChoice ch;
    const int deg = pl.fast_deg;
    if (c.schedule == DVBS2HIP_SCHED_NATURAL) {
        if (!pl.fast) { ch.error = "the natural-order schedule is implemented for codes with check degree <= 27"; return ch; }
        // sum-product in the reference's sweep order: one lane per frame
        if (pl.spa) return pick(ch, LF_NAT_SPA, {deg, pl.spa_rule == 2 ? 2 : 1, 0}, 64, 0, 0);
        // Form by the size of the batch.  Codes whose second hazard plane is empty and whose check count divides by eight (every DVB-S2 code of the library) run CONSECUTIVE CHECKS
        // side by side (ldpc_nat_ck_kernel).  (round 5) While the batch gives every CU at most ONE workgroup of 16 frames (4096 frames on 256 CUs: the BASELINE batch): 8 checks x 8
        // frames per wave, TWO waves per workgroup -- the sweep's step time follows the number of cache lines the waves of a CU touch per group of checks (every slot of every check
        // is one line access per wave whatever the row holds), and rows of 32 frames (the two forms below) put four waves on half the CUs at this size: 4096 normal frames 35.3 -> 24.9-26.8
        // ms = 115 -> 153-165 k frames/s, 1024 frames 31.4 -> 19.3 ms; with two such workgroups on a CU the time doubles (6144 frames: 47.5 against 36.5 ms), so from there on
        // 4 checks x 16 frames, two waves per workgroup = rows of 32 frames (8192 frames: 217 k; 16384+: 245-260 k; one lane per frame reached 171 k at 32768).  Any other code: one lane per
        // frame when that alone gives every SIMD a wave, else a check's edges over 4 or 8 lanes.
        bool plane2_empty = true;      // the second hazard plane is empty: loads may run NAT_AHEAD checks ahead
        for (size_t i = pl.nat_haz.size() / 2; i < pl.nat_haz.size(); i++) plane2_empty &= pl.nat_haz[i] == 0u;
        const bool clean = plane2_empty && pl.M % 8 == 0;
        int parts = clean ? (c.F <= 8 * c.n_cus ? 81 : c.F <= 16 * c.n_cus ? 82 : c.F >= 3072 ? 44 : 88)      // (one wave per CU while that holds the batch: 2048 normal frames 20.9 -> 19.4 ms)
                          : c.F >= 32768 ? 1 : c.F > 6144 ? 4 : 8;
        if (const char *ev = getenv("DVBS2HIP_NAT_PARTS")) { const int v = atoi(ev); if (v == 1 || v == 4 || v == 8 || ((v == 88 || v == 44 || v == 82 || v == 81 || v == 48 || v == 41) && clean)) parts = v; }
        // (two digits: 88 and 44 are the forms above, whose rows hold 32 frames; 82 = <8, 2> and 41 = <4, 1>: rows of 16 frames, twice the workgroups; 81 = <8, 1>: rows of 8; 48 = <4, 4>: rows of 64)
        static const int ck_forms[6][3] = {{88, 8, 4}, {44, 4, 2}, {82, 8, 2}, {81, 8, 1}, {48, 4, 4}, {41, 4, 1}};      // DVBS2HIP_NAT_PARTS code, CK, WV
        for (const int *f : ck_forms)
            if (parts == f[0]) return pick(ch, LF_NAT_CK, {deg, f[1], f[2]}, 64 * f[2], (size_t)pl.q * deg * 8, 0);
        if (parts > 1) {
            const int ahead = parts == 8 ? NAT_AHEAD : NAT_AHEAD / 2;
            return pick(ch, LF_NAT_PART, {deg, parts, plane2_empty && pl.M % ahead == 0 ? ahead : 1}, 64, (size_t)pl.q * ((deg + parts - 1) / parts) * parts * 8, 0);
        }
        return pick(ch, LF_NAT_LANE, {deg, 0, 0}, 64, 0, 0);
    }
    if (!(pl.fast && pl.fast_wg8)) return pick(ch, LF_GENERIC, {pl.ent_stride == 13 ? 13 : LDPC_MAX_SLOTS, pl.hybrid, pl.c2v_lds}, LDPC_THREADS, pl.lds_bytes, 0);
    // (round 6) a call of at most one frame per CU on a code whose image and packed state fit the LDS can run on the two-lanes-per-check kernel (k_ldpc_lat.hip) -- OPT-IN:
    // bit-exact, and measured SLOWER than the lone workgroup of k_ldpc_wg8.hip (one 32APSK-S 3/4 frame: 210 against 177 us; QPSK-S 8/9: 178 against 141).  It reads the LDS-only
    // min-sum plan's tables, whose offsets assume the image's rows in bit-group order; it writes the packed hard decisions only, the BCH stage does the rest.
    // A plan it cannot take stays on k_ldpc_wg8.hip.
    const size_t lat_lds = (size_t)(pl.n_groups + 2) * LDPC_LAT_ROW + (size_t)pl.M * 12 + 16;      // image + junk + inf rows, packed state, one flag word
    const int lat_t[3] = {deg, 0, 0};
    if (env_is("DVBS2HIP_LDPC_LAT", '1') && c.F <= c.n_cus && c.lat_lds_ok && pl.fast_mode == 0 && !pl.spa && lat_lds <= 160 * 1024 - 512 && ldpc_lat_has(lat_t) &&
        pl.w8_lds_junk == (uint32_t)(pl.n_groups * LDPC_LAT_ROW))
        return pick(ch, LF_LAT, lat_t, LDPC_LAT_THREADS, lat_lds, 1);
    // the throughput kernels can write the chain's output socket themselves (descrambled info bits of a frame the BCH stage leaves alone); k_ldpc_wg8.hip can (round 5) also check
    // the BCH remainder of what it outputs, and the BCH stage then decodes the flagged frames only.  (round 6) With the stopping rule their work queue can take a frame order.
    ch.writes_info = !getenv("DVBS2HIP_CHAIN_UNFUSED");
    ch.takes_order = c.early_stop && c.F >= (pl.fast_cu1 ? 2 : 4) * (long long)c.n_cus && env_is("DVBS2HIP_LDPC_ORDER", '1');
    if (pl.fast_cu1) {
        pick(ch, LF_CU1, {deg, pl.spa_rule == 3 ? 3 : pl.spa ? 1 : 0, 0}, LDPC_CU1_THREADS, (size_t)pl.w8_lds_bytes, 1);
        if (ch.error.empty() && pl.cu1_pairs != 2 * ldpc_cu1_nrg()) ch.error = "LDPC: the plan's row pairs do not fill the row-keeping waves of ldpc_cu1_kernel";
        return ch;
    }
    ch.writes_bch = ch.writes_info && c.syn_tables && !env_is("DVBS2HIP_CHAIN_SYN", '0');
    const int rule = pl.spa_rule == 2 || pl.spa_rule == 3 ? pl.spa_rule : pl.spa ? 1 : 0;
    return pick(ch, LF_WG8, {deg, pl.fast_mode, rule}, LDPC_WG8_THREADS, (size_t)pl.w8_lds_bytes, 2);
}

std::string ldpc_choice_name(const LdpcChoice &ch)
{
    if (!ch.error.empty()) return ch.error;
    const std::string d = std::to_string(ch.targ[0]);
    char buf[96];
    switch (ch.family) {
    case LF_NAT_SPA: return "ldpc_nat_spa_kernel<" + d + "," + std::to_string(ch.targ[1]) + ">";
    case LF_NAT_LANE: case LF_NAT_PART: case LF_NAT_CK:      // (one name for the handle, whatever the batch: one lane per frame from 32768 frames on, a check's edges over 4 / 8 lanes below)
        return "ldpc_nat_kernel<" + d + "> / ldpc_nat_part_kernel<" + d + ",4|8> / ldpc_nat_ck_kernel<" + d + ",8|4,1|2|4> by batch size";
    case LF_LAT: return "ldpc_lat_kernel<" + d + ">";
    case LF_GENERIC: snprintf(buf, sizeof buf, "ldpc_layered_nms_kernel<%d,%s,%s>", ch.targ[0], ch.targ[1] ? "true" : "false", ch.targ[2] ? "true" : "false"); return buf;
    case LF_CU1: return ch.targ[1] ? "ldpc_cu1_kernel<" + d + "," + std::to_string(ch.targ[1]) + ">" : "ldpc_cu1_kernel<" + d + ">";
    default: break;
    }
    if (ch.targ[2]) snprintf(buf, sizeof buf, "ldpc_wg8_kernel<%d,%d,%d>", ch.targ[0], ch.targ[1], ch.targ[2]);
    else snprintf(buf, sizeof buf, "ldpc_wg8_kernel<%d,%d>", ch.targ[0], ch.targ[1]);
    return buf;
}

void ldpc_plan_params(const LdpcPlan &pl, LdpcKParams &p)
{
    p.N = pl.N; p.K = pl.K; p.M = pl.M; p.q = pl.q; p.n_info = pl.n_info; p.n_groups = pl.n_groups;
    p.w8.tab = pl.d_w8_tab; p.w8.rows = pl.d_w8_rows;
    p.w8.st_base = pl.w8_st_base; p.w8.lds_junk = pl.w8_lds_junk; p.w8.lds_bytes = pl.w8_lds_bytes;
    p.w8.nl_info = pl.w8_nl_info; p.w8.nl = pl.w8_nl; p.w8.ng_info = pl.w8_ng_info; p.w8.ng = pl.w8_ng;
    p.spa_cap = pl.spa_rule == 3 ? LDPC_SPA_CAP : INFINITY;
}

hipError_t ldpc_launch(const LdpcPlan &pl, const LdpcChoice &ch, LdpcKParams p, float *nat_work, hipStream_t s)
{
    if (!ch.error.empty()) return hipErrorInvalidValue;
    switch (ch.family) {
    case LF_GENERIC: return ldpc_generic_launch(pl, ch, p, s);
    case LF_WG8: return ldpc_wg8_launch(pl, p, s);
    case LF_CU1: return ldpc_cu1_launch(pl, ch, p, s);
    case LF_LAT: return ldpc_lat_launch(pl, ch, p, s);
    default: return ldpc_nat_launch(pl, ch, p, nat_work, s);
    }
}

int ldpc_blocks_per_cu(const LdpcPlan &pl, const LdpcChoice &ch)
{
    if (!ch.error.empty()) return 1;
    return ch.family == LF_WG8 ? ldpc_wg8_blocks_per_cu(pl) : ch.family == LF_GENERIC ? ldpc_generic_blocks_per_cu(pl, ch) : ch.blocks_per_cu > 0 ? ch.blocks_per_cu : 1;
}

}  // namespace dvbs2
