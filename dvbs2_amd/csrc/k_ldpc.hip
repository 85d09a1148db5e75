// a1 -- DVB-S2 LDPC decoder, horizontal-layered normalised min-sum, for gfx950: the host-side PLAN.
//
// Replaces the decoder behind tools::Codec_LDPC<B,Q>::get_decoder_siho()
// (/root/reference src/common/Factory/DVBS2/DVBS2.cpp:418-449, type "BP_HORIZONTAL_LAYERED",
// implem "NMS").  Not a port of AFF3CT's SIMD decoder: that one sweeps the checks of one
// frame serially (inter-frame SIMD only).  Here ONE FRAME = ONE WORKGROUP and
// the code's quasi-cyclic structure gives the intra-frame parallelism:
//
//   * the M = 360 q checks split into q LAYERS {c : c mod q = r}; inside a layer the 360
//     checks (t = c div q) touch every bit-group through a circulant: check t reads element
//     (t - t0) mod 360 of the group, so lane t's accesses are unit-stride across lanes
//     (conflict-free LDS banks / fully coalesced global segments);
//   * posteriors live on chip: as many 360-element bit-groups as fit are kept in LDS
//     (all of them for N = 16200); for N = 64800 (259 KB fp32 > 160 KB LDS) the
//     least-touched groups spill to a per-frame global workspace that stays L2/MALL hot;
//   * check->variable messages are stored COMPRESSED per check: the two output
//     magnitudes, 27 sign bits and the 5-bit position of the minimum = 12 bytes per check
//     instead of 4 bytes per edge, and decompress bit-exactly to the fp32 messages.
//
// This file holds the plan and nothing else: layer tables, storage policy and the choice between the kernels.  ldpc_build_plan runs it as a sequence of
// stages (build_plan_impl at the end of the file); the layout of what they emit is ldpc_layer_table.h.  Every DVB-S2 code shipped here runs on
// k_ldpc_wg8.hip (NMS / MS / SPA; mode 6 of the min-sum decoder: k_ldpc_cu1.hip); the GENERIC table-driven kernel (k_ldpc_generic.hip) is the fallback
// for codes the fast kernels reject -- check degree above 27 or more than 16 duplicate edges per layer.
//
// Schedule and arithmetic are restated in oracle/dvbs2_oracle.c (ORC_SCHED_QC) and the two
// must agree bit for bit: tests/test_ldpc_gpu.py.  The plan itself is seeded and deterministic: tests/test_plan_digest.py pins every table it emits.
#include "dvbs2hip_internal.h"
#include "ldpc_layer_table.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>

namespace dvbs2 {
namespace {

const char *const PLAN_RETRY_GENERIC = "\x01generic";

// Tuning / experiment knobs (environment, read ONCE per ldpc_build_plan, i.e. when a handle is created: the fast attempt and the generic retry see the same values):
//   DVBS2HIP_LDPC_PATH=generic        force the generic kernel
//   DVBS2HIP_LDPC_FAST_MODE=lds|global|static|park|park4|cu1   posterior image of the fast kernels (default: lds for N = 16200; for N = 64800 the static hybrid with rows
//                                     parked in the idle waves' registers (park), static = without them, park4 = mode 4 for the min-sum kernel too)
//   DVBS2HIP_LDPC_LOCK_DUPS=0         static hybrid without forcing the duplicate-edge bit-groups into LDS (then the generic kernel runs)
//   DVBS2HIP_LDPC_C2V=lds|global, DVBS2HIP_LDPC_LDS_GROUPS=n   generic kernel storage policy
//   DVBS2HIP_LDPC_SLOT_ALIGN / _PAD (bytes)   where a workgroup's global slot starts -- measured without effect (docs/negative_results.md), kept for experiments
//   DVBS2HIP_VERBOSE                  says on stderr why an image mode was not used
// (DVBS2HIP_LDPC_BLOCKS_PER_CU, DVBS2HIP_LDPC_GRID_MAX, DVBS2HIP_LDS_LIMIT -- occupancy / scaling experiments -- are read where the handle is made, not here.)
struct PlanKnobs {
    enum Mode { MODE_DEFAULT, MODE_LDS, MODE_GLOBAL /* and any other word */, MODE_STATIC, MODE_PARK, MODE_PARK4, MODE_CU1 };
    enum C2v { C2V_AUTO, C2V_LDS, C2V_GLOBAL /* and any other word */ };
    bool path_generic = false;
    Mode mode = MODE_DEFAULT;
    bool lock_dups = true;
    C2v c2v = C2V_AUTO;
    bool has_lds_groups = false;
    int lds_groups = 0;
    size_t slot_align_words = 1, slot_pad_words = 0;
    bool verbose = false;
    bool mode_hybrid() const { return mode == MODE_STATIC || mode == MODE_PARK || mode == MODE_PARK4; }      // static: hybrid without parked rows; park: the default for the long codes
};

PlanKnobs plan_knobs_from_env()
{
    PlanKnobs k;
    auto is = [](const char *v, const char *w) { return v && !strcmp(v, w); };
    k.path_generic = is(getenv("DVBS2HIP_LDPC_PATH"), "generic");
    if (const char *m = getenv("DVBS2HIP_LDPC_FAST_MODE"))
        k.mode = is(m, "lds") ? PlanKnobs::MODE_LDS : is(m, "static") ? PlanKnobs::MODE_STATIC : is(m, "park") ? PlanKnobs::MODE_PARK : is(m, "park4") ? PlanKnobs::MODE_PARK4 :
                 is(m, "cu1") ? PlanKnobs::MODE_CU1 : PlanKnobs::MODE_GLOBAL;
    if (const char *el = getenv("DVBS2HIP_LDPC_LOCK_DUPS")) k.lock_dups = atoi(el) != 0;
    if (const char *c = getenv("DVBS2HIP_LDPC_C2V")) k.c2v = is(c, "lds") ? PlanKnobs::C2V_LDS : PlanKnobs::C2V_GLOBAL;
    if (const char *g = getenv("DVBS2HIP_LDPC_LDS_GROUPS")) { k.has_lds_groups = true; k.lds_groups = atoi(g); }
    if (const char *ea = getenv("DVBS2HIP_LDPC_SLOT_ALIGN")) k.slot_align_words = (size_t)atoi(ea) / 4;
    if (const char *ep = getenv("DVBS2HIP_LDPC_SLOT_PAD")) k.slot_pad_words = (size_t)atoi(ep) / 4;
    k.verbose = getenv("DVBS2HIP_VERBOSE") != nullptr;
    return k;
}

// One slot of a layer = one circulant of the layer's 360 checks: element (t - t0) mod 360 of the bit-group; lvl: how many edges of the same bit-group stand in front
// of it in the layer (table order); mask0: absent for check 0.  group -1: a NULL slot (padding).
struct Slot { int group, t0, lvl, mask0; };
typedef std::vector<std::vector<Slot>> Layers;        // [q], real slots only, in table order: information edges, p_c, p_{c-1}
typedef std::vector<std::vector<int>> Mult;           // [n_groups][q]: edges of the bit-group in the layer

Mult multiplicities(const Layers &layers, int n_groups)
{
    const int q = (int)layers.size();
    Mult mult(n_groups, std::vector<int>(q, 0));
    for (int r = 0; r < q; r++) for (const Slot &sl : layers[r]) mult[sl.group][r]++;
    return mult;
}

// the two seeded generators of the plan's searches (their sequences are part of the plan: tests/test_plan_digest.py)
struct XorShift32 { uint32_t s = 2463534242u; uint32_t operator()() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s >> 4; } };
struct Lcg32 { uint32_t s = 12345u; uint32_t operator()() { s = s * 1664525u + 1013904223u; return s >> 8; } };

// A set of bit-groups that is to give EVERY layer exactly NL of its slots (the kernels then know at compile time which slots are LDS accesses), at most `cap` rows.
// Greedy fill by the caller, then a randomised local search on sum_r (NL - count_r)^2: swap moves, a worse one accepted now and then.
struct BalancedSet {
    const Mult *mult;
    int q, NL, cap;
    std::vector<char> in;
    std::vector<int> cnt;
    int size = 0;
    BalancedSet(const Mult &m, int q_, int NL_, int cap_) : mult(&m), q(q_), NL(NL_), cap(cap_), in(m.size(), 0), cnt(q_, 0) {}
    bool fits(int g) const { for (int r = 0; r < q; r++) if (cnt[r] + (*mult)[g][r] > NL) return false; return true; }
    void add(int g, int s) { in[g] = s > 0; size += s; for (int r = 0; r < q; r++) cnt[r] += s * (*mult)[g][r]; }
    int cost() const { int c = 0; for (int r = 0; r < q; r++) c += (NL - cnt[r]) * (NL - cnt[r]); return c; }
    // returns the cost reached (0: balanced); `pinned` rows never leave, `banned` ones never enter
    template <class Rnd>
    int search(Rnd &rnd, int max_it, const std::vector<char> &pinned, const std::vector<char> &banned)
    {
        const int n_groups = (int)in.size();
        int c0 = cost();
        for (int it = 0; it < max_it && c0 > 0; it++) {
            int g_out = -1, g_in = -1;
            if (rnd() & 1) { do { g_out = (int)(rnd() % n_groups); } while (!in[g_out]); if (pinned[g_out]) g_out = -1; }
            if (rnd() % 10 != 0) { do { g_in = (int)(rnd() % n_groups); } while (in[g_in] || banned[g_in]); }
            if (g_out >= 0) add(g_out, -1);
            bool ok = true;
            if (g_in >= 0) { ok = fits(g_in) && size < cap; if (ok) add(g_in, +1); }
            const int c1 = ok ? cost() : 1 << 30;
            if (ok && (c1 <= c0 || rnd() % 500 == 0)) c0 = c1;
            else { if (ok && g_in >= 0) add(g_in, -1); if (g_out >= 0) add(g_out, +1); }
        }
        return c0;
    }
};

// ------------------------------------------------------------------------------------------
// MODE 4 ("parked rows", k_ldpc_wg8.hip): on-chip bit-groups = LDS rows + rows PARKED in the registers of the workgroup's two
// idle waves while no layer needs them.  The schedule is static and cyclic over the q layers of an iteration:
//   * the on-chip set S gives every layer exactly NL (14 or 15) of its slots (k_ldpc_wg8.hip knows at compile time which slots
//     are LDS accesses);
//   * n_pos LDS positions, NR = |S| - n_pos of them each shared by a PAIR of rows (X, Y) with register slot k: while X is in the
//     position Y sits in the slot, and twice per iteration the idle waves swap them ("during layer s": between the end-of-layer
//     barriers s-1 and s).  A pair is compatible when two layers s1, s2 that use neither row separate the layers that use X
//     (all inside (s1, s2)) from those that use Y (all inside (s2, s1)): X is swapped in during s1 -- it is first needed by s1 + 1
//     at the earliest -- and out during s2, after its last use;
//   * the other rows of S own a position for good.  Pairs = a matching in the compatibility graph (randomised greedy, restarts).
// Everything here is host code; the result is verified by simulating one full cycle before it is used.
struct ParkPlan {
    std::vector<char> in_chip;              // [n_groups]
    std::vector<std::vector<int>> pos;      // [n_groups][q]: LDS position of the row during layer r (-1: not in LDS then)
    std::vector<uint32_t> srv;              // [q][NR]: LDS position slot k swaps with during layer r (LT_SWAP_NONE: none)
    std::vector<int> lds0, reg0;            // state at the start of layer 0: bit-group at LDS position / in register slot (-1: empty)
    int n_pos = 0, nl0 = 0, n_moves = 0, n_pairs = 0;
};
struct ParkEdge { int x, y, s1, s2; };      // a compatible pair: x in LDS during (s1, s2), y during (s2, s1)

// (A) the on-chip set: exactly NL slots of every layer, at most cap = n_pos + NRmax rows; `seed` holds the doubly connected groups, which stay
bool on_chip_set(BalancedSet &set, const BalancedSet &seed, const std::vector<int> &touches, const std::vector<char> &dup, const std::vector<char> &banned, XorShift32 &rnd)
{
    const int n_groups = (int)seed.in.size();
    set = seed;
    for (;;) {
        int best = 0, bg = -1;
        for (int g = 0; g < n_groups && set.size < set.cap; g++) if (!set.in[g] && !banned[g] && set.fits(g) && touches[g] * 16 + (int)(rnd() % 16) > best) { best = touches[g] * 16 + 15; bg = g; }
        if (bg < 0) break;
        set.add(bg, +1);
    }
    return set.search(rnd, 600000, dup, banned) == 0;
}

// (B) compatible pairs among the rows of S and their swap layers
std::vector<ParkEdge> compatible_pairs(const Mult &mult, const std::vector<int> &S, int q)
{
    std::vector<ParkEdge> edges;
    auto used_by = [&](int g, int l) { return mult[g][((l % q) + q) % q] > 0; };
    for (size_t i = 0; i < S.size(); i++) for (size_t j = i + 1; j < S.size(); j++) {
        const int x = S[i], y = S[j];
        int bs1 = -1, bs2 = -1, bsc = -1;
        for (int s1 = 0; s1 < q; s1++) {
            if (used_by(x, s1) || used_by(y, s1) || used_by(y, s1 + 1)) continue;          // y leaves during s1: not needed in s1 nor s1 + 1 .. ; x arrives
            for (int d = 1; d < q; d++) {
                const int s2 = (s1 + d) % q;
                if (used_by(x, s2) || used_by(y, s2) || used_by(x, s2 + 1)) continue;
                bool okp = true;
                for (int l = 0; l < q && okp; l++) {
                    const bool inside = ((l - s1) % q + q) % q < d;                      // l in [s1, s2)
                    if (used_by(x, l) && !inside) okp = false;
                    if (used_by(y, l) && inside) okp = false;
                }
                if (!okp) continue;
                // slack: layers between the swap and the first use after it (the more, the less a late swap can delay a layer)
                int f1 = 1, f2 = 1;
                while (!used_by(x, s1 + f1)) f1++;
                while (!used_by(y, s2 + f2)) f2++;
                const int sc = std::min(f1, f2);
                if (sc > bsc) { bsc = sc; bs1 = s1; bs2 = s2; }
            }
        }
        if (bs1 >= 0) edges.push_back({x, y, bs1, bs2});
    }
    return edges;
}

// A MAXIMUM matching of the graph `adj` (Edmonds' blossom algorithm), grown from the matching `mate` comes with (-1: unmatched).
void max_matching(const std::vector<std::vector<int>> &adj, std::vector<int> &mate)
{
    const int V = (int)adj.size();
    std::vector<int> par(V), base(V), qu;
    std::vector<char> used(V), blossom(V);
    auto lca = [&](int a, int b) {
        std::vector<char> seen(V, 0);
        for (;;) { a = base[a]; seen[a] = 1; if (mate[a] < 0) break; a = par[mate[a]]; }
        for (;;) { b = base[b]; if (seen[b]) return b; b = par[mate[b]]; }
    };
    auto mark_path = [&](int v, int b, int child) {
        while (base[v] != b) { blossom[base[v]] = blossom[base[mate[v]]] = 1; par[v] = child; child = mate[v]; v = par[mate[v]]; }
    };
    auto find_path = [&](int root) -> int {
        std::fill(used.begin(), used.end(), 0); std::fill(par.begin(), par.end(), -1);
        for (int i = 0; i < V; i++) base[i] = i;
        qu.clear(); qu.push_back(root); used[root] = 1;
        for (size_t qh = 0; qh < qu.size(); qh++) {
            const int v = qu[qh];
            for (int to : adj[v]) {
                if (base[v] == base[to] || mate[v] == to) continue;
                if (to == root || (mate[to] >= 0 && par[mate[to]] >= 0)) {
                    const int cb = lca(v, to);
                    std::fill(blossom.begin(), blossom.end(), 0);
                    mark_path(v, cb, to); mark_path(to, cb, v);
                    for (int i = 0; i < V; i++) if (blossom[base[i]]) { base[i] = cb; if (!used[i]) { used[i] = 1; qu.push_back(i); } }
                } else if (par[to] < 0) {
                    par[to] = v;
                    if (mate[to] < 0) return to;
                    used[mate[to]] = 1; qu.push_back(mate[to]);
                }
            }
        }
        return -1;
    };
    for (int v = 0; v < V; v++) if (mate[v] < 0 && !adj[v].empty()) {
        int u = find_path(v);
        while (u >= 0) { const int pv = par[u], ppv = mate[pv]; mate[u] = pv; mate[pv] = u; u = ppv; }
    }
}

// (C) matching (indices into `edges`): randomised greedy, low-degree rows first; if that falls short, a MAXIMUM matching started from the greedy one (the graph has a
//     few hundred vertices) -- mode 6 needs 72 disjoint pairs among the 160 information rows of the N = 64800 8/9 code and greedy finds 71
std::vector<int> match_pairs(const std::vector<ParkEdge> &edges, int n_groups, int need, XorShift32 &rnd)
{
    std::vector<int> best_match;
    for (int attempt = 0; attempt < 3000 && (int)best_match.size() < need; attempt++) {
        std::vector<int> deg(n_groups, 0), order(edges.size());
        std::vector<uint32_t> key(edges.size());
        for (const ParkEdge &e : edges) { deg[e.x]++; deg[e.y]++; }
        for (size_t i = 0; i < edges.size(); i++) { order[i] = (int)i; key[i] = (uint32_t)(deg[edges[i].x] + deg[edges[i].y]) * 64u + rnd() % (attempt == 0 ? 1u : 512u); }
        std::sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
        std::vector<char> taken(n_groups, 0);
        std::vector<int> m;
        for (int i : order) if (!taken[edges[i].x] && !taken[edges[i].y]) { taken[edges[i].x] = taken[edges[i].y] = 1; m.push_back(i); }
        if (m.size() > best_match.size()) best_match = m;
        if (attempt >= 40 && need > 45) break;      // (many pairs wanted: leave the rest to the exact algorithm)
    }
    if ((int)best_match.size() < need) {
        const int V = n_groups;
        std::vector<std::vector<int>> adj(V);
        std::vector<std::vector<int>> eid(V, std::vector<int>(V, -1));
        for (size_t i = 0; i < edges.size(); i++) { adj[edges[i].x].push_back(edges[i].y); adj[edges[i].y].push_back(edges[i].x); eid[edges[i].x][edges[i].y] = eid[edges[i].y][edges[i].x] = (int)i; }
        std::vector<int> mate(V, -1);
        for (int i : best_match) { mate[edges[i].x] = edges[i].y; mate[edges[i].y] = edges[i].x; }
        max_matching(adj, mate);
        best_match.clear();
        for (int v = 0; v < V; v++) if (mate[v] > v) best_match.push_back(eid[v][mate[v]]);
    }
    return best_match;
}

// (D) tables: positions 0 .. need-1 are the shared ones (slot k <-> position k, pair k = edges[match[k]]), then the rows that own theirs
bool park_tables(ParkPlan &out, const std::vector<char> &inS, const std::vector<int> &S, const std::vector<ParkEdge> &edges, const std::vector<int> &match, int q, int n_pos, int NRmax,
                 std::string &why)
{
    const int n_groups = (int)inS.size(), need = (int)match.size();
    out.in_chip = inS; out.n_pos = n_pos; out.n_pairs = need; out.n_moves = 4 * need;
    out.pos.assign(n_groups, std::vector<int>(q, -1));
    out.srv.assign((size_t)q * NRmax, LT_SWAP_NONE);
    out.lds0.assign(n_pos, -1); out.reg0.assign(NRmax, -1);
    std::vector<char> paired(n_groups, 0);
    for (int k = 0; k < need; k++) {
        const ParkEdge &e = edges[match[k]];
        paired[e.x] = paired[e.y] = 1;
        const int d = ((e.s2 - e.s1) % q + q) % q;
        for (int l = 0; l < q; l++) {
            const int off = ((l - e.s1) % q + q) % q;
            if (off >= 1 && off < d) out.pos[e.x][l] = k;            // x: layers strictly between s1 and s2
            if (off > d) out.pos[e.y][l] = k;                       // y: strictly between s2 and s1
        }
        out.srv[(size_t)e.s1 * NRmax + k] = (uint32_t)k;
        out.srv[(size_t)e.s2 * NRmax + k] = (uint32_t)k;
        // start of layer 0 (before its swaps): x holds the position iff 0 is in (s1, s2]
        const int o0 = ((0 - e.s1) % q + q) % q;
        const bool x_in = o0 >= 1 && o0 <= d;
        out.lds0[k] = x_in ? e.x : e.y; out.reg0[k] = x_in ? e.y : e.x;
    }
    int P = need;
    for (int g : S) if (!paired[g]) { for (int l = 0; l < q; l++) out.pos[g][l] = P; out.lds0[P] = g; P++; }
    if (P > n_pos) { why = "internal: positions"; return false; }
    out.nl0 = P;
    return true;
}

// (E) one full cycle simulated from that state: every access finds its row, no swap touches a row in use, the state closes
bool simulate_cycle(const ParkPlan &out, const Mult &mult, const std::vector<int> &S, int q, int NRmax, std::string &why)
{
    std::vector<int> lds = out.lds0, reg = out.reg0;
    for (int r = 0; r < q; r++) {
        for (int g : S) if (mult[g][r]) { const int Pg = out.pos[g][r]; if (Pg < 0 || lds[Pg] != g) { why = "simulation: row not where the table says"; return false; } }
        for (int k = 0; k < NRmax; k++) {
            const uint32_t e = out.srv[(size_t)r * NRmax + k];
            if (e == LT_SWAP_NONE) continue;
            const int a = lds[e], b = reg[k];
            if (a < 0 || b < 0) { why = "simulation: swap with an empty place"; return false; }
            if (mult[a][r] || mult[a][(r + 1) % q] || mult[b][r]) { why = "simulation: swap of a row in use"; return false; }
            lds[e] = b; reg[k] = a;
        }
    }
    if (lds != out.lds0 || reg != out.reg0) { why = "simulation: the cycle does not close"; return false; }
    return true;
}

bool plan_parked(const Mult &mult, const std::vector<char> &banned, int q, int NL, int n_pos, int NRmax, bool verbose, ParkPlan &out, std::string &why)
{
    const int n_groups = (int)mult.size();
    // the row-keeping waves hand their NRmax rows back through LDS positions 0 .. NRmax-1 at the end of a frame (w8_park_server, cu1_keeper): there have to be that many
    if (n_pos < NRmax) { why = "fewer LDS positions than parked rows (DVBS2HIP_LDS_LIMIT too small for this mode)"; return false; }
    XorShift32 rnd;
    std::vector<int> touches(n_groups, 0);
    std::vector<char> dup(n_groups, 0);
    for (int g = 0; g < n_groups; g++) for (int r = 0; r < q; r++) { touches[g] += mult[g][r]; dup[g] |= mult[g][r] > 1; }
    BalancedSet seed(mult, q, NL, n_pos + NRmax), set = seed;       // the doubly connected groups are in every round's set
    for (int g = 0; g < n_groups; g++) if (dup[g]) {
        if (banned[g] || !seed.fits(g) || seed.size >= seed.cap) { why = "doubly connected bit-groups do not fit"; return false; }
        seed.add(g, +1);
    }
    for (int round = 0; round < 8; round++) {
        if (!on_chip_set(set, seed, touches, dup, banned, rnd)) { why = "no on-chip set with the same number of slots in every layer"; continue; }
        std::vector<int> S;
        for (int g = 0; g < n_groups; g++) if (set.in[g]) S.push_back(g);
        const int need = std::max(0, (int)S.size() - n_pos);    // pairs (= register slots) needed
        if (need > NRmax) { why = "on-chip set too large"; continue; }
        const std::vector<ParkEdge> edges = compatible_pairs(mult, S, q);
        std::vector<int> match = match_pairs(edges, n_groups, need, rnd);
        if (verbose) fprintf(stderr, "[dvbs2hip] plan_parked: %zu rows on chip, %zu compatible pairs, matching %zu of %d needed\n", S.size(), edges.size(), match.size(), need);
        if ((int)match.size() < need) { why = "not enough compatible pairs of rows"; continue; }
        match.resize((size_t)need);
        return park_tables(out, set.in, S, edges, match, q, n_pos, NRmax, why) && simulate_cycle(out, mult, S, q, NRmax, why);
    }
    return false;
}

// ------------------------------------------------------------------------------------------
// the stages of build_plan_impl
// ------------------------------------------------------------------------------------------
// validation; the layers' slots, degrees and conflict levels; E
std::string parse_layers(LdpcPlan &pl, Layers &layers, int N, int K, int n_rows, const int32_t *row_ptr, const int32_t *addr)
{
    if (N <= 0 || K <= 0 || K >= N) return "LDPC: need 0 < K < N";
    const int M = N - K;
    if (M % LDPC_Z || K % LDPC_Z) return "LDPC: N-K and K must be multiples of 360";
    if (n_rows != K / LDPC_Z) return "LDPC: address table must have K/360 rows";
    const int q = M / LDPC_Z;
    pl.N = N; pl.K = K; pl.M = M; pl.q = q; pl.n_info = n_rows; pl.n_groups = n_rows + q;
    for (int i = 0; i < row_ptr[n_rows]; i++)
        if (addr[i] < 0 || addr[i] >= M) return "LDPC: address out of range";

    layers.assign(q, std::vector<Slot>());
    for (int g = 0; g < n_rows; g++)
        for (int p = row_ptr[g]; p < row_ptr[g + 1]; p++) {
            const int r = addr[p] % q, t0 = addr[p] / q;
            int lvl = 0;
            for (const Slot &s : layers[r]) {
                if (s.group == g) { lvl++; if (s.t0 == t0) return "LDPC: duplicate edge in address table"; }
            }
            if (lvl > 3) return "LDPC: more than 4 edges of one bit-group in one layer";
            layers[r].push_back({g, t0, lvl, 0});
        }
    for (int r = 0; r < q; r++) {
        layers[r].push_back({n_rows + r, 0, 0, 0});                 // p_c
        if (r > 0) layers[r].push_back({n_rows + r - 1, 0, 0, 0});  // p_{c-1}, same t
        else       layers[r].push_back({n_rows + q - 1, 1, 0, 1});  // p_{c-1} = group q-1, element t-1; absent for c = 0
    }
    pl.deg_max = 0; pl.E = -1;
    pl.layer_deg.assign(q, 0); pl.layer_lvl.assign(q, 0);
    for (int r = 0; r < q; r++) {
        pl.layer_deg[r] = (int)layers[r].size();
        pl.deg_max = std::max(pl.deg_max, pl.layer_deg[r]);
        pl.E += LDPC_Z * pl.layer_deg[r];
        for (const Slot &s : layers[r]) pl.layer_lvl[r] = std::max(pl.layer_lvl[r], s.lvl);
    }
    if (pl.deg_max > LDPC_MAX_SLOTS) return "LDPC: check degree > 27 not supported by the packed message format";
    return "";
}

// storage policy of the generic kernel: which bit-groups live in LDS (the most-touched first), where the packed c->v state lives
struct GenericStorage {
    std::vector<int> touches, order;      // slots per bit-group; the bit-groups by falling number of slots (stable)
    int nl = 0;                           // bit-groups in LDS
};
GenericStorage generic_storage(LdpcPlan &pl, const Layers &layers, const PlanKnobs &knobs, int lds_groups_req, size_t lds_limit)
{
    GenericStorage gs;
    const int M = pl.M;
    gs.touches.assign(pl.n_groups, 0);
    for (const std::vector<Slot> &l : layers) for (const Slot &s : l) gs.touches[s.group]++;
    gs.order.resize(pl.n_groups);
    std::iota(gs.order.begin(), gs.order.end(), 0);
    std::stable_sort(gs.order.begin(), gs.order.end(), [&](int a, int b) { return gs.touches[a] > gs.touches[b]; });

    const size_t c2v_bytes = (size_t)M * 12, grp_bytes = (size_t)LDPC_Z * 4;
    if (knobs.has_lds_groups) lds_groups_req = knobs.lds_groups;
    const size_t all_post = (size_t)pl.n_groups * grp_bytes;
    bool c2v_lds;
    if (knobs.c2v != PlanKnobs::C2V_AUTO) c2v_lds = knobs.c2v == PlanKnobs::C2V_LDS;
    else c2v_lds = (all_post + c2v_bytes <= lds_limit);     // everything on chip when it fits
    if (c2v_lds && c2v_bytes + grp_bytes > lds_limit) c2v_lds = false;
    const size_t avail = lds_limit - (c2v_lds ? c2v_bytes : 0);
    int max_groups = (int)std::min<size_t>(pl.n_groups, avail / grp_bytes);
    int n_lds = (lds_groups_req < 0) ? max_groups : std::min(lds_groups_req, max_groups);
    pl.lds_groups = n_lds; pl.c2v_lds = c2v_lds; pl.hybrid = n_lds < pl.n_groups;

    pl.groups.assign(pl.n_groups, {0, 0});
    int ng = 0;
    for (int i = 0; i < pl.n_groups; i++) {
        const int g = gs.order[i];
        if (i < n_lds) pl.groups[g] = {(uint32_t)(gs.nl++ * LDPC_Z), 1u};
        else           pl.groups[g] = {(uint32_t)(ng++ * LDPC_Z), 0u};
    }
    pl.lds_post_words = gs.nl * LDPC_Z;
    pl.glb_post_words = ng * LDPC_Z;
    pl.gwork_words = pl.glb_post_words + (c2v_lds ? 0 : 3 * M);
    pl.lds_bytes = (size_t)pl.lds_post_words * 4 + (c2v_lds ? c2v_bytes : 0);
    return gs;
}

// The posterior image of the fast kernels (LdpcPlan::fast_mode) and where every bit-group's row lives in it.
//   0: in LDS; 1: in the workgroup's global slot; 3: STATIC hybrid; 4 / 5: static hybrid + rows parked in the idle waves' registers; 6: one frame per CU (k_ldpc_cu1.hip)
struct Image {
    std::vector<char> in_lds;             // [n_groups] hybrid modes: the bit-group is on chip
    ParkPlan park;                        // modes 4 / 5 / 6
    bool cu1 = false, parked = false, hyb = false;      // hyb (3 .. 6): the first NLH slots of every layer are LDS accesses
    int NLH = 0, NRH = 0;                 // LDS slots per layer; register slots of the row-keeping waves
    std::vector<uint32_t> gbase, glds;    // [n_groups] word offset of the row in its store; 1 = the store is LDS  (parked modes: the LDS position of a row depends on the layer, park.pos)
    int n_l = 0, n_g = 0;                 // hybrid modes: rows in LDS / in the global slot
    int lrows = 0;                        // rows of the LDS image in front of its junk row
};

// mode 6 (k_ldpc_cu1.hip): ONE frame per CU, the whole posterior image on chip -- n_pos LDS positions + the rows parked in the registers of the
// workgroup's four row-keeping waves (two groups of two waves, ldpc_cu1_nrg() rows each); every slot of every layer is an LDS access.  Parity groups
// pair like information groups (the 160 information rows of the N = 64800 8/9 code have a maximum matching of 71 pairs, 72 are needed): a parity row
// that starts an iteration in a register slot is loaded by its row-keeping wave (a stride-q gather), the others by the working waves' scatter.
bool try_one_frame_per_cu(const LdpcPlan &pl, const Mult &mult, int maxdup, size_t lds_limit, bool verbose, ParkPlan &park, std::string &why)
{
    const int q = pl.q;
    const int n_pos = ((int)lds_limit - LDPC_CU1_XCHG_BYTES - 128) / (LDPC_Z * 4) - 1;      // [positions | junk row | exchange area | misc]
    const std::vector<char> banned(pl.n_groups, 0);
    why = "more rows than positions and register slots";
    const int need = pl.n_groups - n_pos;
    return n_pos >= 2 * q && need <= 2 * ldpc_cu1_nrg() && maxdup <= LDPC_CU1_HA - 2 && need > 0 &&
           plan_parked(mult, banned, q, pl.fast_deg, n_pos, 2 * ldpc_cu1_nrg(), verbose, park, why) && park.n_pairs == need;
}

// mode 3 (STATIC hybrid, normal frames): pick the LDS-resident bit-groups so that EVERY layer has exactly NL = 9 of its 27 slots in LDS; the kernel then
// knows at compile time which slots are LDS accesses.  Greedy fill + randomised local search (deterministic seed).  Sets pl.w8_dups_in_lds.
bool static_hybrid_set(LdpcPlan &pl, const Mult &mult, const GenericStorage &gs, const std::vector<char> &banned, bool lock_dups, int cap, std::vector<char> &in_lds)
{
    BalancedSet set(mult, pl.q, 9, cap);
    // bit-groups with two edges in one layer go in first and stay: the duplicate-edge replay and the
    // store redirection of k_ldpc_wg8.hip then never leave LDS (DVBS2HIP_LDPC_LOCK_DUPS=0 to compare)
    std::vector<char> locked(pl.n_groups, 0);
    bool lock_ok = lock_dups;
    std::vector<int> dups;
    for (int g = 0; g < pl.n_groups && lock_ok; g++) {
        bool d = false;
        for (int r = 0; r < pl.q; r++) d |= mult[g][r] > 1;
        if (d) { if (banned[g]) lock_ok = false; dups.push_back(g); }
    }
    for (int g : dups) { if (!lock_ok) break; if (set.fits(g) && set.size < cap) { set.add(g, +1); locked[g] = 1; } else lock_ok = false; }
    if (!lock_ok) { for (int g = 0; g < pl.n_groups; g++) if (set.in[g]) set.add(g, -1); std::fill(locked.begin(), locked.end(), 0); }
    pl.w8_dups_in_lds = lock_ok;
    for (;;) {
        int best = 0, bg = -1;
        for (int i = 0; i < pl.n_groups && set.size < cap; i++) {
            const int g = gs.order[i];
            if (set.in[g] || banned[g] || !set.fits(g)) continue;
            if (gs.touches[g] > best) { best = gs.touches[g]; bg = g; }
        }
        if (bg < 0) break;
        set.add(bg, +1);
    }
    Lcg32 rnd;
    if (set.search(rnd, 400000, locked, banned) != 0) { pl.w8_dups_in_lds = false; return false; }
    in_lds = set.in;
    return true;
}

// modes 0 / 1 / 3 / 4 / 5 / 6: sets pl.fast_mode (and w8_dups_in_lds, pl.groups) and places the rows.  DVBS2HIP_LDPC_FAST_MODE forces a mode where the code allows it.
Image choose_image(LdpcPlan &pl, const Layers &layers, const GenericStorage &gs, const PlanKnobs &knobs, size_t lds_limit, int maxdup, bool small_batch)
{
    const bool spa = pl.spa;
    const size_t grp_bytes = (size_t)LDPC_Z * 4;
    const int n_rows = pl.n_info;
    const int xrows = pl.fast_pad ? 1 : 0;        // the +inf row
    const bool by_env = knobs.mode != PlanKnobs::MODE_DEFAULT, env_hyb = knobs.mode_hybrid(), env_cu1 = knobs.mode == PlanKnobs::MODE_CU1;
    Image im;
    im.in_lds.assign(pl.n_groups, 0);
    // LDS when a CU holds two frames of it (N = 16200), else the workgroup's global slot, upgraded below to the static hybrid where the code allows
    pl.fast_mode = ((size_t)(pl.n_groups + 1 + xrows) * grp_bytes * 2 <= lds_limit + 1024) ? 0 : 1;
    if (by_env && !env_hyb) pl.fast_mode = (knobs.mode == PlanKnobs::MODE_LDS && pl.fast_mode == 0) ? 0 : 1;      // (so `cu1` on a code with an LDS-only image selects mode 1)
    const bool full_deg = pl.fast_deg == 27 && !pl.fast_pad;
    const Mult mult = multiplicities(layers, pl.n_groups);
    // mode 6 where asked for, and
    // (round 6) ... of the min-sum decoder on a handle made for at most one frame per CU (`small_batch`): a call is then one frame's ten iterations on one CU, and
    // with two lanes per check those take 0.42 ms instead of 0.54 (F = 1 .. 256, same box; bit-identical results)
    if ((env_cu1 || (!by_env && !spa && (LDPC_CU1_DEFAULT || small_batch)) || (!by_env && spa && LDPC_CU1_SPA_DEFAULT)) && pl.spa_rule != 2 && pl.fast_mode == 1 && full_deg) {
        std::string why;
        if (try_one_frame_per_cu(pl, mult, maxdup, lds_limit, knobs.verbose, im.park, why)) {
            pl.fast_mode = 6;
            for (int g = 0; g < pl.n_groups; g++) im.in_lds[g] = 1;
            pl.w8_dups_in_lds = true;
        } else if (knobs.verbose || env_cu1) fprintf(stderr, "[dvbs2hip] LDPC plan: mode 6 (one frame per CU) not used (%s)\n", why.c_str());
    }
    if (pl.fast_mode != 6 && (env_hyb || env_cu1 || (!by_env && pl.fast_mode == 1)) && full_deg) {
        const int cap = (int)(lds_limit / 2 / grp_bytes) - 1;            // two frames per CU, one junk row each
        // the parity groups stay out of LDS: table order then puts p_c and p_{c-1} at the last two (global) slots of every layer,
        // where k_ldpc_wg8.hip forwards the parity chain in a register; p_{c-1} of layer 0 is the absent-for-check-0 slot
        std::vector<char> banned(pl.n_groups, 0);
        for (int g = 0; g < pl.n_groups; g++) banned[g] = g >= n_rows;
        if (static_hybrid_set(pl, mult, gs, banned, knobs.lock_dups, cap, im.in_lds)) pl.fast_mode = 3;
        // modes 4 / 5: rows parked in the idle waves' registers on top of the LDS rows (DVBS2HIP_LDPC_FAST_MODE=static keeps mode 3, park4 mode 4
        // for the min-sum kernel too)
        if (pl.fast_mode == 3 && pl.w8_dups_in_lds && knobs.mode != PlanKnobs::MODE_STATIC) {
            std::string why;
            for (int m = (spa || knobs.mode == PlanKnobs::MODE_PARK4) ? 4 : 5; m >= 4 && pl.fast_mode == 3; m--) {
                if (plan_parked(mult, banned, pl.q, ldpc_park_nl(m), cap, ldpc_park_nr(m), knobs.verbose, im.park, why)) {
                    pl.fast_mode = m;
                    for (int g = 0; g < pl.n_groups; g++) im.in_lds[g] = im.park.in_chip[g];
                } else if (knobs.verbose) fprintf(stderr, "[dvbs2hip] LDPC plan: mode %d (parked rows) not used (%s)\n", m, why.c_str());
            }
        }
    }
    im.cu1 = pl.fast_mode == 6;
    im.parked = pl.fast_mode == 4 || pl.fast_mode == 5 || im.cu1; im.hyb = pl.fast_mode == 3 || im.parked;
    im.NLH = im.cu1 ? pl.fast_deg : im.parked ? ldpc_park_nl(pl.fast_mode) : 9; im.NRH = im.cu1 ? 2 * ldpc_cu1_nrg() : ldpc_park_nr(pl.fast_mode);
    im.gbase.assign(pl.n_groups, 0u); im.glds.assign(pl.n_groups, 0u);
    if (im.hyb) {
        for (int g = 0; g < pl.n_groups; g++) {
            if (im.in_lds[g]) { im.gbase[g] = (uint32_t)(im.n_l++ * LDPC_Z); im.glds[g] = 1u; }
            else im.gbase[g] = (uint32_t)(im.n_g++ * LDPC_Z);
        }
    } else
        for (int g = 0; g < pl.n_groups; g++) { im.gbase[g] = (uint32_t)(g * LDPC_Z); im.glds[g] = pl.fast_mode == 0 ? 1u : 0u; }
    for (int g = 0; g < pl.n_groups; g++) pl.groups[g] = {im.gbase[g], im.glds[g]};
    im.lrows = pl.fast_mode == 0 ? pl.n_groups : pl.fast_mode == 3 ? im.n_l : im.parked ? im.park.n_pos : 0;
    return im;
}

// The slots of layer r in the order the kernel of the image takes them (three orderings), NULL-padded to fast_deg.  Conflict levels were fixed in table
// order and travel with the slot.
std::string order_layer_slots(std::vector<Slot> &ord, const LdpcPlan &pl, const Layers &layers, const Image &im, int r)
{
    const int q = pl.q, n_rows = pl.n_info;
    const std::vector<Slot> &ls = layers[r];
    ord.clear();
    auto parity_last = [&]() {
        const size_t nn = ord.size();
        return nn >= 2 && ord[nn - 2].group == n_rows + r && ord[nn - 1].group == n_rows + (r + q - 1) % q && ord[nn - 2].t0 == 0 && (r == 0 || ord[nn - 1].t0 == 0);
    };
    if (im.cu1) {      // one frame per CU: duplicate edges first (level, then table order; conflict entry i is slot i: all in the first half-check's slots), then the
                       // other information slots, p_c and p_{c-1} last (parity chain forwarded in a register by the second half-check's lanes)
        for (int lvl = 1; lvl <= 3; lvl++) for (const Slot &sl : ls) if (sl.lvl == lvl) ord.push_back(sl);
        for (const Slot &sl : ls) if (sl.lvl == 0 && sl.group < n_rows) ord.push_back(sl);
        for (const Slot &sl : ls) if (sl.lvl == 0 && sl.group >= n_rows) ord.push_back(sl);
        if ((int)ord.size() != pl.fast_deg || !parity_last()) return "LDPC: internal: mode 6 needs p_c and p_{c-1} at the last two slots";
    } else if (im.hyb) {      // static hybrid: the LDS-resident slots first (exactly 9 of them; 14 with parked rows), then the others
        // (sum-product kernel: the duplicate edges first, in the order of the conflict list, so that conflict entry i is slot i as in the LDS-only image)
        if (pl.spa) for (int lvl = 1; lvl <= 3; lvl++) for (const Slot &sl : ls) if (im.in_lds[sl.group] && sl.lvl == lvl) ord.push_back(sl);
        for (const Slot &sl : ls) if (im.in_lds[sl.group] && !(pl.spa && sl.lvl > 0)) ord.push_back(sl);
        if ((int)ord.size() != im.NLH) return "LDPC: internal: static hybrid balance broken";
        for (const Slot &sl : ls) if (!im.in_lds[sl.group]) ord.push_back(sl);
        if (!parity_last()) return "LDPC: internal: static hybrid needs p_c and p_{c-1} at the last two slots (parity chain forwarding)";
    } else {
        // EARLY slots first (bit-group not touched by the previous layer, cyclically), then the late ones; the absent-for-check-0 parity slot stays last.
        // In front of them the duplicate edges (the only slots whose stores are redirected: ldpc_w8_kd), never the masked slot (a parity group: no duplicates),
        // in the order of the conflict list (level, then table order): conflict entry i is slot i, which the sum-product layer relies on
        std::vector<char> prev_touch(pl.n_groups, 0);
        for (const Slot &sl : layers[(r + q - 1) % q]) prev_touch[sl.group] = 1;
        for (int lvl = 1; lvl <= 3; lvl++) for (const Slot &sl : ls) if (sl.lvl == lvl) ord.push_back(sl);
        for (const Slot &sl : ls) if (sl.lvl == 0 && !prev_touch[sl.group]) ord.push_back(sl);
        for (const Slot &sl : ls) if (sl.lvl == 0 && prev_touch[sl.group]) ord.push_back(sl);
    }
    if (!ord.empty() && ls.back().mask0 && !ord.back().mask0) return "LDPC: internal: masked slot must stay last";
    // NULL slots (group -1): behind the duplicate edges at the front of the layer in the LDS-only image (like those, their stores are redirected:
    // ldpc_w8_kd), else in front of the last real slot; the last real slot keeps position fast_deg-1 either way
    size_t nd = 0;
    while (nd < ord.size() && ord[nd].lvl > 0) nd++;
    while ((int)ord.size() < pl.fast_deg) ord.insert(pl.fast_mode == 0 ? ord.begin() + (long)nd : ord.end() - 1, Slot{-1, 0, 0, 0});
    return "";
}

// the entry of a slot in layer r; park_bad: a parked row is not in LDS in a layer that uses it
uint32_t pack_slot(const Slot &sl, int r, const LdpcPlan &pl, const Image &im, bool &park_bad)
{
    if (sl.group < 0) return lt_pack_entry(0u, (uint32_t)(pl.fast_mode == 0 ? (im.lrows + 1) * LDPC_Z * 4 : LDPC_Z * 4), false);      // the +inf row
    const bool il = pl.fast_mode == 0 || (im.hyb && im.glds[sl.group]);
    // k_ldpc_wg8.hip image layout -- LDS: [rows | junk | +inf]; global: [junk | +inf | rows]
    uint32_t base = il ? im.gbase[sl.group] * 4u : 2u * LDPC_Z * 4u + im.gbase[sl.group] * 4u;
    if (il && im.parked) { const int P = im.park.pos[sl.group][r]; if (P < 0) park_bad = true; base = (uint32_t)(P < 0 ? 0 : P) * LDPC_Z * 4u; }
    return lt_pack_entry((uint32_t)(sl.t0 * 4), base, il);
}

// the q layer tables (ldpc_layer_table.h).  kd_ok: the LDS-only image's contract that every slot from ldpc_w8_kd(deg) on is a primary edge
std::string emit_layer_table(LdpcPlan &pl, const Layers &layers, const Image &im, bool &park_bad, bool &kd_ok)
{
    const int q = pl.q;
    pl.w8_tab.assign((size_t)q * LDPC_FAST_STRIDE, 0u);
    park_bad = false; kd_ok = true;
    std::vector<Slot> ord;
    for (int r = 0; r < q; r++) {
        uint32_t *T8 = &pl.w8_tab[(size_t)r * LDPC_FAST_STRIDE];
        uint32_t prim = 0, dupmask = 0; int nc = 0;
        const std::string e = order_layer_slots(ord, pl, layers, im, r);
        if (!e.empty()) return e;
        // conflict list sorted by level
        for (int lvl = 1; lvl <= 3; lvl++)
            for (size_t j = 0; j < ord.size(); j++)
                if (ord[j].lvl == lvl && ord[j].group >= 0) {
                    T8[LT_CONF + nc] = pack_slot(ord[j], r, pl, im, park_bad);
                    T8[LT_CONF_META + nc] = lt_pack_meta((uint32_t)j, (uint32_t)lvl);
                    dupmask |= 1u << j;
                    if (im.hyb && !im.glds[ord[j].group]) pl.w8_dups_in_lds = false;
                    nc++;
                }
        for (size_t j = 0; j < ord.size(); j++) {
            T8[j] = pack_slot(ord[j], r, pl, im, park_bad);
            if (ord[j].lvl == 0 && ord[j].group >= 0) prim |= 1u << j;
        }
        T8[LT_PRIM] = prim; T8[LT_CINFO] = (uint32_t)nc; T8[LT_DUPMASK] = dupmask;
        // contract with k_ldpc_wg8.hip: from slot ldpc_w8_kd(deg) on every slot is a primary edge (no redirected store, no NULL slot)
        // (the LDS-only image; with the hybrid image the same trick measured 0.7 % SLOWER on the 15 LDS slots of a normal-frame layer and is not used)
        for (int j = ldpc_w8_kd(pl.fast_deg); j < pl.fast_deg && pl.fast_mode == 0; j++) if (!((prim >> j) & 1u)) kd_ok = false;
        for (int i = 0; i < 2 && i < nc; i++) {
            T8[LT_CINFO] |= lt_cinfo_field(T8[LT_CONF_META + i], i);
            T8[LT_CONF0 + i] = T8[LT_CONF + i];
        }
        if (nc > 0 && lt_meta_lvl(T8[LT_CONF_META]) != 1u) return "LDPC: internal: first conflict entry is not of level 1";
        if (pl.fast_mode == 0 || pl.spa || im.cu1) for (int i = 0; i < nc; i++) if (lt_meta_slot(T8[LT_CONF_META + i]) != (uint32_t)i) return "LDPC: internal: conflict entry i is not slot i";
        if (pl.spa) {
            // the oracle's edge order of a check (information bits in address-table order, p_c, p_{c-1} = layers[r]) as slots: the tanh-product
            // rule multiplies in THAT order (fp32 products do not commute bit for bit); NULL slots (tanh(inf / 2) = 1, exact) fill the tail
            std::vector<int> perm;
            std::vector<char> used(ord.size(), 0);
            for (const Slot &sl : layers[r])
                for (size_t j = 0; j < ord.size(); j++)
                    if (!used[j] && ord[j].group == sl.group && ord[j].t0 == sl.t0) { perm.push_back((int)j); used[j] = 1; break; }
            if ((int)perm.size() != pl.layer_deg[r] || nc > LDPC_TANH_ORDER - LT_CONF_META) return "LDPC: internal: edge-order table";
            for (size_t j = 0; j < ord.size(); j++) if (!used[j]) perm.push_back((int)j);
            for (size_t c = 0; c < perm.size(); c++) T8[LDPC_TANH_ORDER + c / LT_ORDER_PER_DWORD] |= (uint32_t)perm[c] << (LT_ORDER_BITS * (c % LT_ORDER_PER_DWORD));
        }
    }
    return "";
}

// rotated byte offset of check t's element inside the row of an entry
inline uint32_t rotated(uint32_t t, uint32_t shift) { return (t * 4u + (uint32_t)LDPC_Z * 4u - shift) % ((uint32_t)LDPC_Z * 4u); }

// per-lane address table of the min-sum layer (k_ldpc_wg8.hip, ATAB: every slot of the LDS-only image)
void emit_atab_minsum(LdpcPlan &pl)
{
    const int q = pl.q, NW4 = (pl.fast_deg + 3) / 4;
    pl.w8_atab.assign((size_t)q * NW4 * LDPC_AT_LANES * 4, 0u);
    for (int r = 0; r < q; r++) {
        const uint32_t *T8 = &pl.w8_tab[(size_t)r * LDPC_FAST_STRIDE];
        for (int j = 0; j < 4 * NW4; j++)
            for (int t = 0; t < LDPC_AT_LANES; t++) {
                uint32_t v = ATAB_DROPPED;                                       // lanes past the 360th check / padding slots: an offset every buffer access drops
                if (j < pl.fast_deg) {
                    const uint32_t shift = lt_shift(T8[j]), base = lt_base(T8[j]);
                    if (t < LDPC_Z) v = rotated((uint32_t)t, shift) + base;      // (every slot of the LDS-only image is an LDS slot; a NULL slot's entry carries no flag)
                    else v = base;                                              // an LDS slot of an idle lane: any address inside the allocation (never accessed: `act`)
                }
                pl.w8_atab[(((size_t)r * NW4 + j / 4) * LDPC_AT_LANES + t) * 4 + (j & 3)] = v;
            }
    }
}

// (round 5) per-lane address table of the SUM-PRODUCT layer on the LDS-only image (k_ldpc_wg8.hip, AT16): two 16-bit LDS byte addresses per dword (slot 2 k in the low
// half), [q][pieces of 16 bytes][LDPC_AT_LANES][4] -- the image's 45 rows end at byte 64800, so every address of a real slot fits; a NULL slot reads the +inf WORD the
// kernel keeps at junk row + 4 (the +inf row itself lies beyond 64 KB; the junk row is written at its word 0 only in this form), and the slot of check 0's absent
// p_{c-1} points at the junk row's word 0 (its value is replaced by +inf, its store lands there).  false: an address does not fit (no DVB-S2 code: an LDS-only image is 45 rows)
bool emit_atab_spa16(LdpcPlan &pl, const Image &im)
{
    const int q = pl.q, ND = (pl.fast_deg + 1) / 2, NP = (ND + 3) / 4;
    const uint32_t junk = (uint32_t)(im.lrows * LDPC_Z * 4), infw = junk + 4u, inf_row = (uint32_t)((im.lrows + 1) * LDPC_Z * 4);
    bool fits = junk + 8u <= 65536u;
    pl.w8_atab.assign((size_t)q * NP * LDPC_AT_LANES * 4, 0u);
    for (int r = 0; r < q && fits; r++) {
        const uint32_t *T8 = &pl.w8_tab[(size_t)r * LDPC_FAST_STRIDE];
        for (int j = 0; j < pl.fast_deg; j++)
            for (int t = 0; t < LDPC_AT_LANES; t++) {
                const uint32_t shift = lt_shift(T8[j]), base = lt_base(T8[j]);
                uint32_t v = junk;                                                   // idle lanes: never accessed (`act`)
                if (t < LDPC_Z) {
                    if (base == inf_row) v = infw;
                    else if (j == pl.fast_deg - 1 && r == 0 && t == 0) v = junk;
                    else v = rotated((uint32_t)t, shift) + base;
                }
                if (v >= 65536u) fits = false;
                pl.w8_atab[(((size_t)r * NP + (j / 2) / 4) * LDPC_AT_LANES + t) * 4 + ((j / 2) & 3)] |= v << (16 * (j & 1));
            }
    }
    return fits;
}

// bit k - k0 of the mask = register slot k (k0 <= k < k0 + n) swaps during layer r; false: a slot that swaps with another position than its own index
bool swap_mask(unsigned long long &m, const std::vector<uint32_t> &srv, int NR, int r, int k0, int n)
{
    m = 0;
    for (int k = 0; k < n; k++) {
        const uint32_t e = srv[(size_t)r * NR + k0 + k];
        if (e == LT_SWAP_NONE) continue;
        if ((int)e != k0 + k) return false;
        m |= 1ull << k;
    }
    return true;
}

// w8_rows (image rows in storage order, the parity groups' places, the register slots' rows) and, parked modes, the swaps behind the layer tables
std::string emit_rows_and_swaps(LdpcPlan &pl, const Image &im, bool park_bad)
{
    const int q = pl.q;
    const ParkPlan &park = im.park;
    auto on_chip = [&](int g) { return pl.fast_mode == 0 || (im.hyb && im.glds[g]); };
    // LDS rows then global rows (bit-groups ascend inside each: info first)
    std::vector<int> lrow, grow;
    for (int g = 0; g < pl.n_groups; g++) (on_chip(g) ? lrow : grow).push_back(g);
    if (im.parked) {      // LDS rows = the positions that hold a row at the start of an iteration (layer 0), in position order
        if (park_bad) return "LDPC: internal: parked-row table";
        lrow.assign(park.lds0.begin(), park.lds0.begin() + park.nl0);
    }
    pl.w8_nl = (int)lrow.size(); pl.w8_ng = (int)grow.size();
    pl.w8_nl_info = im.cu1 ? (int)lrow.size() : (int)std::count_if(lrow.begin(), lrow.end(), [&](int g) { return g < pl.n_info; });      // (mode 6: parity rows may sit among the pairs' positions; the kernel looks at every position)
    pl.w8_ng_info = (int)std::count_if(grow.begin(), grow.end(), [&](int g) { return g < pl.n_info; });
    pl.w8_rows.clear();
    for (int g : lrow) pl.w8_rows.push_back((uint32_t)g);
    for (int g : grow) pl.w8_rows.push_back((uint32_t)g);
    // then, for the frame input of the parity part: where parity group r (bit-group n_info + r) lives
    for (int r = 0; r < q; r++) {
        const int g = pl.n_info + r;
        if (on_chip(g) && im.parked && !im.cu1) return "LDPC: internal: parity group among the parked rows";
        if (im.cu1) {      // where the parity group is at the start of an iteration: byte offset of its LDS position, or in a register slot
            uint32_t where = ROWS_NONE;
            for (int P = 0; P < park.nl0; P++) if (park.lds0[P] == g) where = (uint32_t)(P * LDPC_Z * 4);
            pl.w8_rows.push_back(where);
            continue;
        }
        pl.w8_rows.push_back(on_chip(g) ? (uint32_t)im.gbase[g] * 4u : ROWS_GLOBAL | (uint32_t)((2 * LDPC_Z + (int)im.gbase[g]) * 4));      // global slot: [junk][+inf][rows]
    }
    if (im.parked) {      // then the bit-group in register slot k of the row-keeping waves at the start of an iteration
        for (int k = 0; k < im.NRH; k++) pl.w8_rows.push_back(park.reg0[k] < 0 ? (uint32_t)ROWS_NONE : (uint32_t)park.reg0[k]);
        // and the swaps behind the layer tables: [q][NR] x LDS position, then the same as 64-bit masks -- the row-keeping waves test a bit per slot instead of
        // loading and comparing a table entry per slot (39 dependent scalar loads per layer).  Modes 4 / 5 (round 4): one mask per layer; mode 6: one per
        // layer and group of row-keeping waves, bit k = slot k of the group
        pl.w8_tab.insert(pl.w8_tab.end(), park.srv.begin(), park.srv.end());
        const int n_grp = im.cu1 ? 2 : 1, per = im.NRH / n_grp;
        for (int r = 0; r < q; r++) for (int gk = 0; gk < n_grp; gk++) {
            unsigned long long m;
            if (!swap_mask(m, park.srv, im.NRH, r, gk * per, per))
                return im.cu1 ? "LDPC: internal: mode 6 expects pair k at position k" : "LDPC: internal: parked rows: pair k is expected at position k";
            pl.w8_tab.push_back((uint32_t)m); pl.w8_tab.push_back((uint32_t)(m >> 32));
        }
    } else
        for (size_t i = 0; i < lrow.size(); i++) if ((int)im.gbase[lrow[i]] != (int)i * LDPC_Z) return "LDPC: internal: LDS row order";
    for (size_t i = 0; i < grow.size(); i++) if ((int)im.gbase[grow[i]] != (int)i * LDPC_Z) return "LDPC: internal: global row order";
    return "";
}

// LDS bytes and the workgroup's global slot: [posteriors kept in global memory | packed c->v state 3 M words]
void size_workspace(LdpcPlan &pl, const Image &im, const PlanKnobs &knobs)
{
    const int M = pl.M, xrows = pl.fast_pad ? 1 : 0;
    const bool spa = pl.spa, cu1 = im.cu1;
    const int n_lds_rows = im.parked ? im.park.n_pos : pl.w8_nl;
    pl.w8_lds_junk = (uint32_t)(n_lds_rows * LDPC_Z * 4);
    pl.w8_lds_bytes = (n_lds_rows + 1 + (pl.fast_pad && pl.fast_mode == 0 ? 1 : 0)) * LDPC_Z * 4 + LDPC_W8_MISC_BYTES;
    pl.w8_park_moves = im.parked ? im.park.n_moves : 0;
    pl.w8_st_base = (uint32_t)((2 + pl.w8_ng) * LDPC_Z * 4);
    pl.w8_gwork_words = (2 + pl.w8_ng) * LDPC_Z + 3 * M;
    if (cu1) {      // LDS: [positions | junk row | exchange area of the two half-checks | misc]; global: the packed state alone, 16 bytes per check {c1, c2, pk of half A, pk of half B}
        pl.w8_lds_bytes = (n_lds_rows + 1) * LDPC_Z * 4 + LDPC_CU1_XCHG_BYTES + 128;
        pl.w8_st_base = 0u;
        pl.w8_gwork_words = 4 * M;
        pl.cu1_pairs = im.park.n_pairs;
    }
    if (spa) pl.w8_gwork_words = (2 + pl.w8_ng) * LDPC_Z + pl.fast_deg * M;      // SPA: one fp32 message per edge slot, [layer][slot][360]
    if (spa && cu1) pl.w8_gwork_words = pl.fast_deg * M;                          // mode 6: the messages alone, [layer][half][group of 4 slots][360][4]
    if (knobs.slot_align_words > 1) pl.w8_gwork_words = (int)(((size_t)pl.w8_gwork_words + knobs.slot_align_words - 1) / knobs.slot_align_words * knobs.slot_align_words);
    pl.w8_gwork_words += (int)knobs.slot_pad_words;
    pl.glb_post_words = pl.fast_mode == 1 ? (pl.n_groups + xrows) * LDPC_Z : im.hyb ? im.n_g * LDPC_Z : 0;
    pl.lds_post_words = pl.fast_mode == 0 ? (pl.n_groups + 1 + xrows) * LDPC_Z : pl.fast_mode == 3 ? (im.n_l + 1) * LDPC_Z : im.parked ? (im.park.n_pos + 1) * LDPC_Z : 0;
    if (cu1) pl.glb_post_words = 0;
    // +inf row: LDS image = [groups | junk row | inf row]; global image = [groups | inf row]
    pl.fast_inf_row = pl.fast_pad ? (pl.n_groups + (pl.fast_mode == 0 ? 1 : 0)) * LDPC_Z * 4 : -1;
    pl.gwork_words = pl.glb_post_words + (spa ? pl.fast_deg * M : cu1 ? 4 * M : 3 * M);      // SPA: one fp32 message per edge slot
    pl.lds_bytes = (size_t)pl.lds_post_words * 4;
    pl.hybrid = im.hyb; pl.c2v_lds = false; pl.lds_groups = pl.fast_mode == 0 ? pl.n_groups : im.n_l;
}

// k_ldpc_nat.hip (natural row order, one lane per frame): per layer the info slots (NULL-padded), then p_c, then p_{c-1}; and the hazard planes
std::string emit_nat_tables(LdpcPlan &pl, const Layers &layers)
{
    const int q = pl.q, M = pl.M, K = pl.K;
    pl.nat_tab.assign((size_t)q * pl.fast_deg * 2, 0u);
    for (int r = 0; r < q; r++) {
        uint32_t *T = &pl.nat_tab[(size_t)r * pl.fast_deg * 2];
        const std::vector<Slot> &ls = layers[r];           // table order: info edges, p_c, p_{c-1}
        const int n_real = (int)ls.size(), n_null = pl.fast_deg - n_real;
        int j = 0;
        auto put = [&](const Slot &sl) {
            const bool par = sl.group >= pl.n_info;
            T[2 * j] = (uint32_t)sl.t0 | (par ? (uint32_t)NAT_PARITY : 0u);
            T[2 * j + 1] = par ? (uint32_t)(K + (sl.group - pl.n_info)) : (uint32_t)(sl.group * LDPC_Z);
            j++;
        };
        for (int i = 0; i < n_real - 2; i++) put(ls[i]);
        for (int i = 0; i < n_null; i++) { T[2 * j] = NAT_NULL; T[2 * j + 1] = 0u; j++; }
        put(ls[n_real - 2]); put(ls[n_real - 1]);
        if (ls[n_real - 2].group != pl.n_info + r || !(ls[n_real - 1].group >= pl.n_info)) return "LDPC: internal: parity slots are not last";
    }
    // first plane: consecutive checks (cyclically) that share a bit other than the forwarded p_{c-1}
    // second plane (behind the first): check c shares a bit with one of the NAT_HAZ_WINDOW checks before it (cyclically) -- the kernels that request a
    // check's posteriors several checks ahead (k_ldpc_nat.hip, ldpc_nat_part_kernel: NAT_AHEAD checks) must not do so for these: the checks in between
    // have not written yet, and the stores of the one or two before them may still be in flight
    const size_t hw = (size_t)(M + 31) / 32;
    pl.nat_haz.assign(2 * hw, 0u);
    auto vars_of = [&](int c, std::vector<int> &out) {
        out.clear();
        const int r = c % q, t = c / q;
        for (const Slot &sl : layers[r]) {
            if (sl.mask0 && c == 0) continue;
            const int e = ((t - sl.t0) % LDPC_Z + LDPC_Z) % LDPC_Z;
            out.push_back(sl.group < pl.n_info ? sl.group * LDPC_Z + e : K + q * e + (sl.group - pl.n_info));
        }
    };
    std::vector<int> a, b;
    for (int c = 0; c < M; c++) {
        vars_of(c, a);
        const int fwd_bit = c > 0 ? K + c - 1 : -1;
        for (int d = 1; d <= NAT_HAZ_WINDOW; d++) {
            vars_of(((c - d) % M + M) % M, b);
            bool hz = false;
            for (int x : a) if (x != fwd_bit && std::find(b.begin(), b.end(), x) != b.end()) hz = true;
            if (hz && d == 1) pl.nat_haz[c >> 5] |= 1u << (c & 31);
            if (hz) pl.nat_haz[hw + (c >> 5)] |= 1u << (c & 31);
        }
    }
    return "";
}

// the generic kernel's entries (LdpcEntry, dvbs2hip_internal.h), from pl.groups as the image left them
std::string emit_generic_entries(LdpcPlan &pl, const Layers &layers, int n_lds_generic)
{
    if (pl.n_groups > 255) return "LDPC: more than 255 bit-groups not supported by the packed entry format";
    pl.ent_stride = pl.deg_max <= 13 ? 13 : LDPC_MAX_SLOTS;
    // padding entries read slot 0 of a store that exists and are ignored
    const LdpcEntry null_entry = LE_NULL | (n_lds_generic > 0 ? LE_LDS : 0u);
    pl.entries.assign((size_t)pl.q * pl.ent_stride, null_entry);
    for (int r = 0; r < pl.q; r++)
        for (size_t j = 0; j < layers[r].size(); j++) {
            const Slot &s = layers[r][j];
            const LdpcGroup &gl = pl.groups[s.group];
            pl.entries[(size_t)r * pl.ent_stride + j] =
                (LdpcEntry)s.t0 | ((gl.base / LDPC_Z) << LE_SLOT_SHIFT) | (gl.lds ? LE_LDS : 0u) |
                (s.mask0 ? LE_MASK0 : 0u) | ((uint32_t)s.lvl << LE_LVL_SHIFT);
        }
    return "";
}

// the fast kernels' plan: regular codes -- uniform check degree (11 or 27) or layers padded to 13 / 27 slots with NULL slots that read a row of +inf and
// store nowhere -- with few same-layer duplicates (maxc of them at most in a layer).  PLAN_RETRY_GENERIC: a code the fast kernels cannot take after all
std::string plan_fast(LdpcPlan &pl, const Layers &layers, const GenericStorage &gs, const PlanKnobs &knobs, size_t lds_limit, bool uniform, int maxc, bool small_batch)
{
    const bool spa = pl.spa;
    pl.fast = true;
    pl.fast_deg = (uniform && pl.deg_max == 11) ? 11 : (uniform && pl.deg_max == 27) ? 27 : pl.deg_max <= 13 ? 13 : 27;
    pl.fast_pad = !(uniform && pl.deg_max == pl.fast_deg);
    const Image im = choose_image(pl, layers, gs, knobs, lds_limit, maxc, small_batch);
    bool park_bad, kd_ok;
    std::string e = emit_layer_table(pl, layers, im, park_bad, kd_ok);
    if (!e.empty()) return e;
    if (!spa && !im.cu1 && pl.fast_mode == 0) emit_atab_minsum(pl);
    if (spa && !im.cu1 && pl.fast_mode == 0 && pl.fast_deg <= LDPC_SPA_AT16_MAXDEG && !emit_atab_spa16(pl, im)) return PLAN_RETRY_GENERIC;
    e = emit_rows_and_swaps(pl, im, park_bad);
    if (!e.empty()) return e;
    size_workspace(pl, im, knobs);
    e = emit_nat_tables(pl, layers);
    if (!e.empty()) return e;
    // one frame per 8-wave workgroup, two independent workgroups per CU (k_ldpc_wg8.hip); a code it cannot take (a static hybrid
    // whose doubly connected bit-groups do not all fit in LDS) goes to the generic table-driven kernel
    const bool w8_ok = (pl.fast_mode == 0 || pl.fast_mode == 1 || (im.hyb && pl.w8_dups_in_lds)) && kd_ok;
    if (!(w8_ok && (size_t)pl.w8_lds_bytes <= lds_limit + 512) || (spa && maxc > LDPC_SPA_MAXC)) return PLAN_RETRY_GENERIC;
    pl.fast_wg8 = true; pl.gwork_words = pl.w8_gwork_words; pl.fast_cu1 = im.cu1;
    return "";
}

std::string build_plan_impl(LdpcPlan &pl, const PlanKnobs &knobs, int N, int K, int n_rows, const int32_t *row_ptr, const int32_t *addr, int lds_groups_req, size_t lds_limit,
                            int spa_rule, bool allow_fast, bool small_batch)
{
    pl.spa = spa_rule != 0; pl.spa_rule = spa_rule;
    Layers layers;
    std::string e = parse_layers(pl, layers, N, K, n_rows, row_ptr, addr);
    if (!e.empty()) return e;
    const GenericStorage gs = generic_storage(pl, layers, knobs, lds_groups_req, lds_limit);
    bool uniform = true;
    int maxc = 0;      // duplicate edges in a layer, at most
    for (int r = 0; r < pl.q; r++) {
        if (pl.layer_deg[r] != pl.deg_max) uniform = false;
        int c = 0;
        for (const Slot &s : layers[r]) c += s.lvl > 0;
        maxc = std::max(maxc, c);
    }
    if (allow_fast && !knobs.path_generic && maxc <= LDPC_FAST_MAXC) {
        e = plan_fast(pl, layers, gs, knobs, lds_limit, uniform, maxc, small_batch);
        if (!e.empty()) return e;
    }
    e = emit_generic_entries(pl, layers, gs.nl);
    if (!e.empty()) return e;
    if (pl.spa && !pl.fast) return "LDPC: SPA is only implemented for codes the fast path accepts (check degree <= 27, at most 6 duplicate edges per layer)";
    return "";
}

}  // namespace

std::string ldpc_build_plan(LdpcPlan &pl, int N, int K, int n_rows, const int32_t *row_ptr,
                            const int32_t *addr, int lds_groups_req, size_t lds_limit, int spa_rule, bool small_batch)
{
    const PlanKnobs knobs = plan_knobs_from_env();
    std::string e = build_plan_impl(pl, knobs, N, K, n_rows, row_ptr, addr, lds_groups_req, lds_limit, spa_rule, true, small_batch);
    if (e == PLAN_RETRY_GENERIC) { pl = LdpcPlan(); e = build_plan_impl(pl, knobs, N, K, n_rows, row_ptr, addr, lds_groups_req, lds_limit, spa_rule, false, small_batch); }
    return e;
}

}  // namespace dvbs2
