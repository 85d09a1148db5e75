// Development aid (CPU, no GPU needed): builds the LDPC plan of a MODCOD exactly as dvbs2hip_create does and prints what the
// static hybrid search chose -- LDS rows, slots per layer, whether the parity chain sits at the last two slots.
//   hipcc -std=c++17 -I dvbs2_amd/csrc -I include tools/plan_probe.cpp -L dvbs2_amd/lib -ldvbs2hip -Wl,-rpath,$PWD/dvbs2_amd/lib -o tools/bin/plan_probe
#include "ldpc_dispatch.h"
#include "ldpc_layer_table.h"
#include "../include/dvbs2hip.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include <cstring>
using namespace dvbs2;

// `plan_probe digest MODCOD SPA_RULE SMALL_BATCH LDS_LIMIT [--fields] [--bad-address]`: one line that pins the whole plan -- the error string, the scalars that choose the
// kernel and size its memory in clear, and one FNV-1a-64 over every host field of LdpcPlan in declaration order (scalars as 64-bit values, vectors as length + contents;
// the device pointers, grid_max and n_cus are not the plan's).  --fields: a line per field, to locate a difference between two builds.  --bad-address: the address table
// with its first entry set to M (an error string's case).  tests/test_plan_digest.py compares the lines with tests/golden/ldpc_plan_digests.json.
struct Fnv {
    unsigned long long h = 0xcbf29ce484222325ull;
    void bytes(const void *p, size_t n) { const unsigned char *b = (const unsigned char *)p; for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; } }
    void scalar(long long v) { bytes(&v, sizeof v); }
};
static int digest_main(int argc, char **argv)
{
    bool fields = false, bad = false;
    std::vector<const char *> a;
    for (int i = 2; i < argc; i++) { if (!strcmp(argv[i], "--fields")) fields = true; else if (!strcmp(argv[i], "--bad-address")) bad = true; else a.push_back(argv[i]); }
    if (a.size() != 4) { std::fprintf(stderr, "usage: plan_probe digest MODCOD SPA_RULE SMALL_BATCH LDS_LIMIT [--fields] [--bad-address]\n"); return 2; }
    dvbs2hip_cfg cfg;
    if (dvbs2hip_cfg_from_modcod(a[0], &cfg)) { std::printf("unknown modcod\n"); return 1; }
    std::vector<int32_t> addr(cfg.ldpc_addr, cfg.ldpc_addr + cfg.ldpc_row_ptr[cfg.ldpc_n_rows]);
    if (bad) addr[0] = cfg.N_ldpc - cfg.K_ldpc;
    LdpcPlan pl;
    const std::string e = ldpc_build_plan(pl, cfg.N_ldpc, cfg.K_ldpc, cfg.ldpc_n_rows, cfg.ldpc_row_ptr, addr.data(), cfg.ldpc_lds_groups, (size_t)atol(a[3]), atoi(a[1]), atoi(a[2]) != 0);
    Fnv all;
    auto field = [&](const char *name, const void *p, size_t n, long long len) {
        Fnv f;
        if (len >= 0) { f.scalar(len); all.scalar(len); }
        f.bytes(p, n); all.bytes(p, n);
        if (fields) std::printf("  %-16s %016llx\n", name, f.h);
    };
#define SC(x) do { const long long v__ = (long long)pl.x; field(#x, &v__, sizeof v__, -1); } while (0)
#define VE(x) field(#x, pl.x.data(), pl.x.size() * sizeof pl.x[0], (long long)pl.x.size())
    SC(N); SC(K); SC(M); SC(q); SC(n_info); SC(n_groups); SC(E); SC(deg_max); SC(ent_stride); SC(lds_groups); SC(c2v_lds); SC(hybrid);
    SC(lds_post_words); SC(glb_post_words); SC(gwork_words); SC(lds_bytes);
    VE(entries); VE(layer_deg); VE(layer_lvl); VE(groups);
    SC(fast); SC(spa); SC(spa_rule); SC(fast_deg); SC(fast_pad); SC(fast_inf_row); SC(fast_mode);
    VE(nat_tab); VE(nat_haz);
    SC(fast_cu1); SC(cu1_pairs); SC(fast_wg8); SC(w8_dups_in_lds);
    VE(w8_tab); VE(w8_rows); VE(w8_atab);
    SC(w8_st_base); SC(w8_lds_junk); SC(w8_lds_bytes); SC(w8_gwork_words); SC(w8_nl_info); SC(w8_nl); SC(w8_ng_info); SC(w8_ng); SC(w8_park_moves);
#undef SC
#undef VE
    std::printf("digest: '%s' fast %d fast_deg %d fast_pad %d fast_mode %d fast_wg8 %d fast_cu1 %d w8_nl %d w8_ng %d w8_lds_bytes %d w8_gwork_words %d gwork_words %d lds_bytes %zu fnv %016llx\n",
                e.c_str(), pl.fast, pl.fast_deg, pl.fast_pad, pl.fast_mode, pl.fast_wg8, pl.fast_cu1, pl.w8_nl, pl.w8_ng, pl.w8_lds_bytes, pl.w8_gwork_words, pl.gwork_words, pl.lds_bytes, all.h);
    return 0;
}

// `plan_probe choice MODCOD SPA_RULE SMALL_BATCH LDS_LIMIT N_CUS SCHEDULE:F .. [--bad-address] [--junk-row] [--deg D] [--mode M] [--rule R]`: a line per SCHEDULE:F with the kernel ldpc_choose
// (ldpc_dispatch.h) picks for a call of F frames on that plan (SCHEDULE: qc | natural; early stop on, the fused chain's tables present, a 160 KiB LDS; the DVBS2HIP_* variables as the environment has them) --
// the instantiation as the code object names it, what it writes, its shape, the name the API reports, the error text.  The options doctor the plan first: the junk row one row
// further, another slot count, image mode or sum-product rule.  `plan_probe insts`: every instantiation the families' tables hold.  tests/test_ldpc_dispatch.py reads both.
static std::string symbol(LdpcFamily f, const int *t)
{
    std::string s = std::string(ldpc_family(f).kernel) + "<" + std::to_string(t[0]);
    for (int i = 1; i < ldpc_family(f).n_targ; i++) s += ", " + (f == LF_GENERIC ? std::string(t[i] ? "true" : "false") : std::to_string(t[i]));
    return s + ">";
}
static int choice_main(int argc, char **argv)
{
    std::vector<const char *> a;
    int junk_rows = 0, deg = -1, mode = -1, rule = -1;
    bool bad = false;
    for (int i = 2; i < argc; i++) {
        if (!strcmp(argv[i], "--junk-row")) junk_rows = 1;
        else if (!strcmp(argv[i], "--bad-address")) bad = true;
        else if (!strcmp(argv[i], "--deg") && i + 1 < argc) deg = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--mode") && i + 1 < argc) mode = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--rule") && i + 1 < argc) rule = atoi(argv[++i]);
        else a.push_back(argv[i]);
    }
    if (a.size() < 6) { std::fprintf(stderr, "usage: plan_probe choice MODCOD SPA_RULE SMALL_BATCH LDS_LIMIT N_CUS qc|natural:F .. [--junk-row] [--deg D] [--mode M] [--rule R]\n"); return 2; }
    dvbs2hip_cfg cfg;
    if (dvbs2hip_cfg_from_modcod(a[0], &cfg)) { std::printf("unknown modcod\n"); return 1; }
    std::vector<int32_t> addr(cfg.ldpc_addr, cfg.ldpc_addr + cfg.ldpc_row_ptr[cfg.ldpc_n_rows]);
    if (bad) addr[0] = cfg.N_ldpc - cfg.K_ldpc;
    LdpcPlan pl;
    const std::string e = ldpc_build_plan(pl, cfg.N_ldpc, cfg.K_ldpc, cfg.ldpc_n_rows, cfg.ldpc_row_ptr, addr.data(), cfg.ldpc_lds_groups, (size_t)atol(a[3]), atoi(a[1]), atoi(a[2]) != 0);
    if (!e.empty()) { std::printf("plan: '%s'\n", e.c_str()); return 0; }      // (no plan, no choice: dvbs2hip_create fails with this text)
    pl.w8_lds_junk += (uint32_t)(junk_rows * LDPC_LAT_ROW);
    if (deg >= 0) pl.fast_deg = deg;
    if (mode >= 0) pl.fast_mode = mode;
    if (rule >= 0) { pl.spa_rule = rule; pl.spa = rule != 0; }
    for (size_t k = 5; k < a.size(); k++) {
        const char *colon = strchr(a[k], ':');
        if (!colon) { std::fprintf(stderr, "'%s' is not SCHEDULE:F\n", a[k]); return 2; }
        const LdpcChoice ch = ldpc_choose(pl, {a[k][0] == 'n' ? DVBS2HIP_SCHED_NATURAL : DVBS2HIP_SCHED_QC, atoi(colon + 1), atoi(a[4]), true, true, true});
        std::printf("choice %s: %s | info %d bch %d order %d | block %d lds %zu per_cu %d | name '%s' | error '%s'\n", a[k], symbol(ch.family, ch.targ).c_str(), ch.writes_info, ch.writes_bch,
                    ch.takes_order, ch.block, ch.lds_bytes, ch.blocks_per_cu, ldpc_choice_name(ch).c_str(), ch.error.c_str());
    }
    return 0;
}
static int insts_main()
{
    for (int f = 0; f < LF_COUNT; f++)
        for (int x = 0; x < 32; x++) for (int y = 0; y < 32; y++) for (int z = 0; z < 32; z++) {
            const int t[3] = {x, y, z};
            const LdpcFamily fam = (LdpcFamily)f;
            const int n = ldpc_family(fam).n_targ;
            if ((n < 3 && z) || (n < 2 && y)) continue;
            if (ldpc_has(fam, t)) std::printf("%s\n", symbol(fam, t).c_str());
        }
    return 0;
}

// `plan_probe syncseg N F CAP [N F CAP ..]`: a line `nseg seg_F` per triple -- how sync_segment_plan (rx_dispatch.h: the function sync_choose calls, the
// handle's scratch present) cuts a one-stream call of F frames of N positions for the average over frames when at most CAP segments are allowed.
// tests/test_sync_seg_plan.py and tests/test_sync_seg_gpu.py read it.
static int syncseg_main(int argc, char **argv)
{
    if (argc < 5 || (argc - 2) % 3) { std::fprintf(stderr, "usage: plan_probe syncseg N F CAP [N F CAP ..]\n"); return 2; }
    for (int i = 2; i + 2 < argc; i += 3) {
        const SyncSegPlan p = sync_segment_plan(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), true);
        std::printf("%d %d\n", p.nseg, p.seg_F);
    }
    return 0;
}

// The receive path's choosers (rx_dispatch.h): a line per case -- the kernel's name as the code object and the results files spell it, then the launch geometry.  The facts
// of a case are integers on the command line (alignments in bytes, flags 0 / 1), several cases one after the other; the DVBS2HIP_* knobs come from the environment.
//   front  BPS SEP ITL_COLS N_SYM PL_FRAME F ALIGN_PL ALIGN_LLR LOCATED FROM_PL DEINTERLEAVE
//   fir    T N_PER S ALIGN_X ALIGN_Y HAVE_FRAG          upfir  T OSF N_IN ALIGN_X ALIGN_Y HAVE_FRAG
//   sync   N FS S ALIGN_X HAVE_FRAG HAVE_SEG ONE_TASK LOCATED   (the delay line of 4 (N + 1) floats every handle has)
//   lr     S N ALIGN_X ALIGN_Y                          walk   K
// tests/test_rx_dispatch.py walks them; the fp64 GPU tests ask which form their cases reach.
static int rx_main(const char *mode, int argc, char **argv)
{
    const int per = !strcmp(mode, "front") ? 11 : !strcmp(mode, "sync") ? 8 : !strcmp(mode, "lr") ? 4 : !strcmp(mode, "walk") ? 1 : 6;
    if (argc < 2 + per || (argc - 2) % per) { std::fprintf(stderr, "usage: plan_probe %s followed by %d integers per case\n", mode, per); return 2; }
    for (int i = 2; i + per <= argc; i += per) {
        long long a[11];
        for (int k = 0; k < per; k++) a[k] = atoll(argv[i + k]);
        if (!strcmp(mode, "front")) {
            const FrontChoice ch = front_choose({(int)a[0], a[1] != 0, (int)a[2], (int)a[3], (int)a[4], (int)a[5], (unsigned)a[6], (unsigned)a[7], a[8] != 0, a[9] != 0, a[10] != 0});
            std::printf("front: %s | block %d grid %d x %d slice_chunk %d\n", front_choice_name(ch).c_str(), ch.block, (int)a[5], ch.grid_y, ch.slice_chunk);
        } else if (!strcmp(mode, "fir") || !strcmp(mode, "upfir")) {
            const FirChoice ch = mode[0] == 'f' ? fir_choose((int)a[0], a[1], (int)a[2], (unsigned)a[3], (unsigned)a[4], a[5] != 0) : upfir_choose((int)a[0], (int)a[1], a[2], (unsigned)a[3], (unsigned)a[4], a[5] != 0);
            std::printf("%s: %s | grid %u x %u tiles_per_wg %d\n", mode, fir_choice_name(ch).c_str(), ch.grid_x, ch.grid_y, ch.family == FIR_MFMA ? ch.tiles_per_wg : 0);
        } else if (!strcmp(mode, "sync")) {
            const SyncFacts c = {(int)a[0], (int)a[1], (int)a[2], 4 * ((int)a[0] + 1), (unsigned)a[3], a[4] != 0, a[5] != 0, a[6] != 0, a[7] != 0};
            const SyncChoice ch = sync_choose(c);
            std::printf("sync: %s grid %u x %d fused %d | %s nwg %d nseg %d seg_F %d | delay line grid %d x %d x %d\n", sync_corr_name(c, ch).c_str(), ch.corr_grid, c.S, ch.fused,
                        sync_argmax_name(ch).c_str(), ch.nwg, ch.seg.nseg, ch.seg.seg_F, ch.vd_gx, ch.vd_gy, c.S);
        } else if (!strcmp(mode, "lr")) {
            const LrChoice ch = lr_choose((int)a[0], (int)a[1], (unsigned)a[2], (unsigned)a[3]);
            std::printf("lr: %s | launches %d timeout_us %llu workgroups per frame %d rotation %s\n", lr_choice_name(ch).c_str(), ch.one_launch ? 1 : 3, ch.timeout_us, ch.cpf,
                        ch.pair ? "sff_rotate2_kernel<0>" : "sff_rotate_kernel<0>");
        } else
            std::printf("walk: %s\n", pls_walk_choose((int)a[0]) ? "pls_walk_lane_kernel" : "pls_walk_double_kernel");
    }
    return 0;
}

int main(int argc, char **argv)
{
    for (const char *m : {"front", "fir", "upfir", "sync", "lr", "walk"})
        if (argc > 1 && !strcmp(argv[1], m)) return rx_main(m, argc, argv);
    if (argc > 1 && !strcmp(argv[1], "syncseg")) return syncseg_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "digest")) return digest_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "choice")) return choice_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "insts")) return insts_main();
    dvbs2hip_cfg cfg;
    if (dvbs2hip_cfg_from_modcod(argc > 1 ? argv[1] : "QPSK-N_8/9", &cfg)) { std::printf("unknown modcod\n"); return 1; }
    LdpcPlan pl;
    const std::string e = ldpc_build_plan(pl, cfg.N_ldpc, cfg.K_ldpc, cfg.ldpc_n_rows, cfg.ldpc_row_ptr, cfg.ldpc_addr, -1, argc > 3 ? atoi(argv[3]) : 160 * 1024, argc > 2 && argv[2][0] == 's');
    std::printf("plan: '%s' fast %d deg %d mode %d wg8 %d dups_in_lds %d | LDS rows %d (info %d) global rows %d (info %d) | lds bytes %d gwork words %d\n", e.c_str(), pl.fast,
                pl.fast_deg, pl.fast_mode, pl.fast_wg8, pl.w8_dups_in_lds, pl.w8_nl, pl.w8_nl_info, pl.w8_ng, pl.w8_ng_info, pl.w8_lds_bytes, pl.w8_gwork_words);
    if (pl.fast_wg8 && (pl.fast_mode == 3 || pl.fast_mode == 4 || pl.fast_mode == 5)) {
        // the static hybrid's contract with the kernel: the first NL slots of every layer (and only those) are LDS accesses
        const int NL = pl.fast_mode == 3 ? 9 : ldpc_park_nl(pl.fast_mode);
        bool ok = true;
        for (int r = 0; r < pl.q; r++) for (int j = 0; j < pl.fast_deg; j++) ok &= lt_is_lds(pl.w8_tab[(size_t)r * LDPC_FAST_STRIDE + j]) == (j < NL);
        int swaps = 0;
        if (pl.fast_mode >= 4) for (size_t i = lt_swaps_at(pl.q); i < lt_swap_masks_at(pl.q, ldpc_park_nr(pl.fast_mode)); i++) swaps += pl.w8_tab[i] != LT_SWAP_NONE;
        std::printf("hybrid: %d LDS slots per layer %s | parked rows %d, row moves per iteration %d, swaps in the table %d\n", NL, ok ? "ok" : "BROKEN", pl.fast_mode >= 4 ? ldpc_park_nr(pl.fast_mode) : 0,
                    pl.w8_park_moves, swaps);
    }
    if (!pl.nat_haz.empty()) {      // natural-order kernels: how many checks the hazard planes flag (plane 0: shares a bit with the check before it; plane 1: with one of the NAT_HAZ_WINDOW before it)
        const size_t hw = pl.nat_haz.size() / 2;
        int n0 = 0, n1 = 0;
        for (size_t i = 0; i < hw; i++) { n0 += __builtin_popcount(pl.nat_haz[i]); n1 += __builtin_popcount(pl.nat_haz[hw + i]); }
        std::printf("natural order: %d of %d checks share a bit with the check before them, %d with one of the %d before them\n", n0, pl.M, n1, NAT_HAZ_WINDOW);
    }
    if (pl.fast_cu1) {
        // mode 6 (k_ldpc_cu1.hip): replay one cycle of the tables as the kernel reads them -- where every slot's row is said to be (LDS position in THAT layer) against
        // a simulation of the row-keeping waves' swaps from the start state (w8_rows: rows at the positions, then the parity groups' positions, then the slots' rows)
        const int q = pl.q, NRT = 2 * ldpc_cu1_nrg(), P = pl.w8_nl;
        std::vector<int> lds(pl.w8_rows.begin(), pl.w8_rows.begin() + P), reg;
        for (int k = 0; k < NRT; k++) reg.push_back((int)pl.w8_rows[(size_t)P + pl.w8_ng + q + k]);
        const std::vector<int> lds0 = lds, reg0 = reg;
        const uint32_t *srv = &pl.w8_tab[lt_swaps_at(q)];
        bool ok = pl.w8_ng == 0 && (int)pl.w8_lds_junk == P * LDPC_Z * 4;
        int swaps = 0, dupmax = 0, seen_rows = 0;
        std::vector<char> seen(pl.n_groups, 0);
        for (int g : lds) if (g >= 0 && g < pl.n_groups && !seen[g]) { seen[g] = 1; seen_rows++; }
        for (int g : reg) if (g >= 0 && g < pl.n_groups && !seen[g]) { seen[g] = 1; seen_rows++; }
        for (int r = 0; r < q && ok; r++) {
            const uint32_t *T = &pl.w8_tab[(size_t)r * LDPC_FAST_STRIDE];
            // slots 25 / 26 are p_c / p_{c-1}; every slot is an LDS access whose base is the position of a row; a slot's row must not be under way
            std::vector<int> used;
            for (int j = 0; j < pl.fast_deg; j++) { const uint32_t base = lt_base(T[j]); ok &= lt_is_lds(T[j]) && base % (LDPC_Z * 4) == 0 && (int)(base / (LDPC_Z * 4)) < P; used.push_back(lds[base / (LDPC_Z * 4)]); }
            ok &= used[pl.fast_deg - 2] == pl.n_info + r && used[pl.fast_deg - 1] == pl.n_info + (r + q - 1) % q;
            const int ncf = (int)lt_ncf(T[LT_CINFO]);
            dupmax = std::max(dupmax, ncf);
            for (int i = 0; i < ncf; i++) ok &= (int)lt_meta_slot(T[LT_CONF_META + i]) == i && i < LDPC_CU1_HA && T[LT_CONF + i] == T[i] && !((T[LT_PRIM] >> i) & 1u);       // conflict entry i is slot i, in half A, not primary
            for (int j = ncf; j < pl.fast_deg; j++) ok &= ((T[LT_PRIM] >> j) & 1u) != 0u;                                                                // every other slot is primary
            // the next layer's rows must already be in place when this layer's swaps run (a swap may take the whole layer), and a swapped row is used by neither
            std::vector<int> next;
            { const uint32_t *Tn = &pl.w8_tab[(size_t)((r + 1) % q) * LDPC_FAST_STRIDE]; (void)Tn; }
            for (int k = 0; k < NRT; k++) {
                const uint32_t e = srv[(size_t)r * NRT + k];
                if (e == LT_SWAP_NONE) continue;
                swaps++;
                ok &= (int)e < P;
                const int a = lds[e], b = reg[k];
                for (int g : used) ok &= g != a && g != b;
                lds[e] = b; reg[k] = a;
            }
        }
        ok &= lds == lds0 && reg == reg0 && seen_rows == pl.n_groups;
        for (int r = 0; r < q; r++) {      // where parity group r starts: its position, or 0xFFFFFFFF and then one of the register slots
            const uint32_t wh = pl.w8_rows[(size_t)P + r];
            if (wh == ROWS_NONE) ok &= std::find(reg0.begin(), reg0.end(), pl.n_info + r) != reg0.end();
            else ok &= wh % (LDPC_Z * 4) == 0 && lds0[wh / (LDPC_Z * 4)] == pl.n_info + r;
        }
        std::printf("cu1: positions %d pairs %d swaps per iteration %d max duplicate edges per layer %d tables %s\n", P, pl.cu1_pairs, swaps, dupmax, ok ? "ok" : "BROKEN");
    }
    if (pl.fast_wg8) {
        for (int r = 0; r < pl.q; r++) {
            const uint32_t *T = &pl.w8_tab[(size_t)r * LDPC_FAST_STRIDE];
            const int ncf = (int)lt_ncf(T[LT_CINFO]);
            std::printf("layer %2d: ncf %d :", r, ncf);
            for (int i = 0; i < ncf; i++) std::printf(" (slot %u lvl %u shift %u)", lt_meta_slot(T[LT_CONF_META + i]), lt_meta_lvl(T[LT_CONF_META + i]), lt_shift(T[LT_CONF + i]) / 4);
            std::printf("  prim %07x\n", T[LT_PRIM]);
        }
    }
    return 0;
}
