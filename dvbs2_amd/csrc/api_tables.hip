// The tables dvbs2hip_create uploads, each built on the host from the configuration and the code plans (declared in dvbs2hip_handle.h).
#include "dvbs2hip_handle.h"

namespace dvbs2 {

void pl_sequence(std::vector<uint8_t> &seq)
{
    // ETSI EN 302 307 5.5.4, n = 0; equals PL_RAND_SEQ (Scrambler_PL.hpp:54-4207)
    const int P = (1 << 18) - 1;
    std::vector<uint8_t> x(P), y(P);
    for (int i = 0; i < 18; i++) { x[i] = i == 0; y[i] = 1; }
    for (int i = 0; i + 18 < P; i++) { x[i + 18] = x[i + 7] ^ x[i]; y[i + 18] = y[i + 10] ^ y[i + 7] ^ y[i + 5] ^ y[i]; }
    seq.resize(66420);
    for (int i = 0; i < 66420; i++) {
        const int i2 = (i + 131072) % P;
        seq[i] = (uint8_t)(2 * (x[i2] ^ y[i2]) + (x[i] ^ y[i]));
    }
}

std::vector<uint32_t> bb_prbs(int K)
{
    // Scrambler_BB.hpp:28 init, Scrambler_BB.hxx:56-64 step
    int l[15] = {1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> out((K + 31) / 32, 0u);
    for (int i = 0; i < K; i++) {
        const int fb = l[14] ^ l[13];
        for (int j = 14; j > 0; j--) l[j] = l[j - 1];
        l[0] = fb;
        if (fb) out[i >> 5] |= 1u << (i & 31);
    }
    return out;
}

static bool prbs_bit(const std::vector<uint32_t> &prbs, int i) { return (prbs[i >> 5] >> (i & 31)) & 1u; }

// the BB scrambler's bits by (bit-group row, wave): two 32-bit words per 64 bits of a 360-bit row (LdpcKParams::info_prbs)
std::vector<uint32_t> bb_prbs_by_row(const dvbs2hip_cfg &cfg, const std::vector<uint32_t> &prbs)
{
    std::vector<uint32_t> rw((size_t)(cfg.K_ldpc / 360) * 6 * 2, 0u);
    for (int i = 0; i < cfg.K_bch; i++)
        if (prbs_bit(prbs, i)) { const int g = i / 360, e = i % 360, w = e >> 6, l = e & 63; rw[(size_t)(g * 6 + w) * 2 + (l >> 5)] |= 1u << (l & 31); }
    return rw;
}

// TX LDPC encoder: per parity layer r (of q) the entries (address / q) | (bit-group << 9), rows padded to `stride`
TxEncTable tx_enc_table(const dvbs2hip_cfg &cfg)
{
    const int M = cfg.N_ldpc - cfg.K_ldpc, q = M / 360;
    std::vector<std::vector<uint32_t>> lay(q);
    for (int g = 0; g < cfg.ldpc_n_rows; g++)
        for (int p = cfg.ldpc_row_ptr[g]; p < cfg.ldpc_row_ptr[g + 1]; p++)
            lay[cfg.ldpc_addr[p] % q].push_back((uint32_t)(cfg.ldpc_addr[p] / q) | ((uint32_t)g << 9));
    TxEncTable t;
    size_t stride = 1;
    for (auto &l : lay) stride = std::max(stride, l.size());
    t.stride = (int)stride;
    t.tab.assign((size_t)q * stride, 0u);
    t.deg.resize(q);
    for (int r = 0; r < q; r++) { t.deg[r] = (int32_t)lay[r].size(); std::copy(lay[r].begin(), lay[r].end(), t.tab.begin() + (size_t)r * stride); }
    return t;
}

// ---- polynomials modulo the BCH generator g(x) of degree r <= 192, as three 64-bit words (bit i = coefficient of x^i)
struct GenPoly {
    unsigned long long g[3] = {0, 0, 0};      // g(x) without its leading term
    int r;
    explicit GenPoly(const std::vector<uint8_t> &gen) : r((int)gen.size() - 1)
    {
        for (int i = 0; i < r; i++) if (gen[i]) g[i / 64] |= 1ull << (i % 64);
    }
};

// v(x) <- (v(x) x + in x^r) mod g(x)
static void xn_mod_g_step(unsigned long long v[3], const GenPoly &gp, unsigned in = 0u)
{
    const int top = gp.r - 1;
    const unsigned fb = (unsigned)((v[top / 64] >> (top % 64)) & 1ull) ^ in;
    v[2] = (v[2] << 1) | (v[1] >> 63); v[1] = (v[1] << 1) | (v[0] >> 63); v[0] <<= 1;
    for (int w = 0; w < 3; w++) {       // keep r bits
        const int lo = 64 * w;
        if (gp.r <= lo) v[w] = 0; else if (gp.r < lo + 64) v[w] &= (1ull << (gp.r - lo)) - 1ull;
    }
    if (fb) { v[0] ^= gp.g[0]; v[1] ^= gp.g[1]; v[2] ^= gp.g[2]; }
}

// byte-wise encoder table: T[u] = (u(x) x^r) mod g(x), u's bit 7 = highest degree
std::vector<unsigned long long> bch_byte_table(const std::vector<uint8_t> &gen)
{
    const GenPoly gp(gen);
    std::vector<unsigned long long> tab(256 * 3, 0ull);
    for (int u = 0; u < 256; u++) {
        unsigned long long *s = &tab[3 * u];
        for (int b = 7; b >= 0; b--) xn_mod_g_step(s, gp, (u >> b) & 1u);
    }
    return tab;
}

// segmented division (tx_bchpar_kernel): segment s of TX_BCH_SEG is followed by after_s bytes; shift[s][b] = x^(b + 8 after_s) mod g
std::vector<unsigned long long> bch_shift_table(const std::vector<uint8_t> &gen, int K_bch)
{
    const GenPoly gp(gen);
    const int SEG = TX_BCH_SEG, r = gp.r, nbytes = K_bch / 8, L = (nbytes + SEG - 1) / SEG;
    std::vector<unsigned long long> sh((size_t)SEG * r * 3, 0ull);
    std::vector<long long> base(SEG);
    long long nmax = 0;
    for (int sgm = 0; sgm < SEG; sgm++) {
        const int b1 = std::min(std::min(sgm * L, nbytes) + L, nbytes);
        base[sgm] = 8ll * (nbytes - b1); nmax = std::max(nmax, base[sgm] + r);
    }
    unsigned long long v[3] = {1ull, 0ull, 0ull};                       // x^n mod g, n = 0, 1, ..
    for (long long n = 0; n < nmax; n++, xn_mod_g_step(v, gp))
        for (int sgm = 0; sgm < SEG; sgm++)
            if (n >= base[sgm] && n < base[sgm] + r) { unsigned long long *d = &sh[((size_t)sgm * r + (size_t)(n - base[sgm])) * 3]; d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; }
    return sh;
}

// tables of the BCH verification inside the LDPC kernel's output phase (k_ldpc_wg8.hip, `syn_tab`): position i = 360 g + t of the BCH word is the
// coefficient of x^(N_bch - 1 - i) = x^(360 (G - 1 - g)) x^(359 - t) (k_bch.hip).  One 32-byte record per row in the kernel's STORAGE order (LDS rows, global
// rows, register slots) {1440 g, last-row flag, A_g = x^(360 (G - 1 - g)) mod g(x)}, then [LDPC_SYN_RED][nsw]: x^k mod g(x) for the once-per-frame reduction;
// 4 (deg g <= 128) or 6 little-endian 32-bit words; and the BB descrambler's bits by (storage row, wave).  Returns an error text, empty when all is well.
std::string ldpc_syn_tables(const dvbs2hip_cfg &cfg, const LdpcPlan &lp, const std::vector<uint8_t> &gen, const std::vector<uint32_t> &prbs, LdpcSynTables &t)
{
    const GenPoly gp(gen);
    const int G = cfg.K_ldpc / 360, nsw = gp.r <= 128 ? 4 : 6;
    const bool parked = lp.fast_mode == 4 || lp.fast_mode == 5;
    const int nrp = parked ? ldpc_park_nr(lp.fast_mode) : 0;
    std::vector<int> order;                       // bit-group of every emitted row (-1: empty register slot)
    for (int l = 0; l < lp.w8_nl_info; l++) order.push_back((int)lp.w8_rows[l]);
    for (int l = 0; l < lp.w8_ng_info; l++) order.push_back((int)lp.w8_rows[lp.w8_nl + l]);
    for (int k = 0; k < nrp; k++) { const uint32_t g = lp.w8_rows[lp.w8_nl + lp.w8_ng + lp.q + k]; order.push_back(g == 0xFFFFFFFFu ? -1 : (int)g); }
    std::vector<int> seen(G, 0);                  // every information row exactly once
    for (int g : order) if (g >= 0 && (g >= G || seen[g]++)) return "internal: LDPC plan emits an information row twice or a parity row";
    for (int g = 0; g < G; g++) if (!seen[g]) return "internal: LDPC plan does not emit every information row";
    const int rows = (int)order.size();
    std::vector<uint32_t> ag((size_t)G * 6, 0u);
    t.pos.assign((size_t)rows * 8 + (size_t)LDPC_SYN_RED * nsw, 0u);
    const int nmax = std::max(360 * (G - 1), LDPC_SYN_RED - 1);
    unsigned long long v[3] = {1ull, 0ull, 0ull};                       // x^n mod g, n = 0, 1, ..
    for (int n = 0; n <= nmax; n++, xn_mod_g_step(v, gp)) {
        auto put = [&](uint32_t *d) {
            d[0] = (uint32_t)v[0]; d[1] = (uint32_t)(v[0] >> 32); d[2] = (uint32_t)v[1]; d[3] = (uint32_t)(v[1] >> 32);
            if (nsw == 6) { d[4] = (uint32_t)v[2]; d[5] = (uint32_t)(v[2] >> 32); }
        };
        if (n % 360 == 0 && n / 360 < G) put(&ag[(size_t)(G - 1 - n / 360) * 6]);
        if (n < LDPC_SYN_RED) put(&t.pos[(size_t)rows * 8 + (size_t)n * nsw]);
    }
    for (int k = 0; k < rows; k++) {
        uint32_t *d = &t.pos[(size_t)k * 8];
        const int g = order[k];
        if (g < 0) { d[0] = 0x7FFFF000u; continue; }
        d[0] = (uint32_t)g * 1440u; d[1] = g == G - 1 ? 1u : 0u;
        for (int i = 0; i < 6; i++) d[2 + i] = ag[(size_t)g * 6 + i];
    }
    // the descrambler's bits per (first row of a batch, lane): bit k of entry [ks][t] = PRBS bit of information bit 360 g + t, g the row emitted at ks + k (k < 16)
    t.prbs_s.assign((size_t)rows * LDPC_AT_LANES, 0u);
    for (int ks = 0; ks < rows; ks++)
        for (int k = 0; k < 16 && ks + k < rows; k++) {
            const int g = order[ks + k];
            if (g < 0) continue;
            for (int e = 0; e < 360; e++) {
                const int i = g * 360 + e;
                if (i < cfg.K_bch && prbs_bit(prbs, i)) t.prbs_s[(size_t)ks * LDPC_AT_LANES + e] |= 1u << k;
            }
        }
    t.words = nsw; t.rows = rows;
    return "";
}

// PLHEADER = 26 SOF + 64 PLS symbols, pi/2-BPSK (Framer.hxx:97-196)
std::vector<float> plheader(const dvbs2hip_cfg &cfg)
{
    static const int G[7][32] = {
        {1,0,0,1,0,0,0,0,1,0,1,0,1,1,0,0,0,0,1,0,1,1,0,1,1,1,0,1,1,1,0,1}, {0,1,0,1,0,1,0,1,0,1,0,1,0,1,0,1,0,1,0,1,0,1,0,1,0,1,0,1,0,1,0,1},
        {0,0,1,1,0,0,1,1,0,0,1,1,0,0,1,1,0,0,1,1,0,0,1,1,0,0,1,1,0,0,1,1}, {0,0,0,0,1,1,1,1,0,0,0,0,1,1,1,1,0,0,0,0,1,1,1,1,0,0,0,0,1,1,1,1},
        {0,0,0,0,0,0,0,0,1,1,1,1,1,1,1,1,0,0,0,0,0,0,0,0,1,1,1,1,1,1,1,1}, {0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1},
        {1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1}};
    static const int SCR[64] = {0,1,1,1,0,0,0,1,1,0,0,1,1,1,0,1,1,0,0,0,0,0,1,1,1,1,0,0,1,0,0,1,0,1,0,1,0,0,1,1,0,1,0,0,0,0,1,0,0,0,1,0,1,1,0,1,1,1,1,1,1,0,1,0};
    static const int SOF[26] = {0,1,1,0,0,0,1,1,0,1,0,0,1,0,1,1,1,0,1,0,0,0,0,0,1,0};
    std::vector<float> plh(180);
    const float a = (float)(1 / std::sqrt(2.0));
    for (int i = 0; i < 13; i++) {
        const int e = 1 - 2 * SOF[2 * i], o = 1 - 2 * SOF[2 * i + 1];
        plh[4 * i] = a * e; plh[4 * i + 1] = a * e; plh[4 * i + 2] = -1 * a * o; plh[4 * i + 3] = a * o;
    }
    for (int i = 0; i < 32; i++) {
        int c = 0;
        for (int r = 0; r < 7; r++) c = (c + (cfg.pls[r] & 1) * G[r][i]) % 2;
        const int e = 1 - 2 * ((c + SCR[2 * i]) % 2), o = 1 - 2 * (((c == 0 ? 1 : 0) + SCR[2 * i + 1]) % 2);
        float *p = &plh[52 + 4 * i];
        if ((cfg.pls[0] & 1) == 0) { p[0] = a * e; p[1] = a * e; p[2] = -1 * a * o; p[3] = a * o; }
        else { p[0] = -1 * a * e; p[1] = a * e; p[2] = -1 * a * o; p[3] = -1 * a * o; }
    }
    return plh;
}

// the constellation normalised to unit mean energy in fp32 (tools::Constellation_user); empty when it has no energy
std::vector<float> unit_constellation(const dvbs2hip_cfg &cfg)
{
    const int P = 1 << cfg.bps;
    std::vector<float> cs(2 * P);
    float es = 0.f;
    for (int i = 0; i < P; i++) es += cfg.cstl[2 * i] * cfg.cstl[2 * i] + cfg.cstl[2 * i + 1] * cfg.cstl[2 * i + 1];
    const float sc = sqrtf(es / (float)P);
    if (!(sc > 0.f)) return {};
    for (int i = 0; i < 2 * P; i++) cs[i] = cfg.cstl[i] / sc;
    return cs;
}

// a separable 2-bit constellation: bit b on one axis alone, two levels, the two bits on different axes => the four points are the product set
bool separable_2bit(const std::vector<float> &cs, int ax[2], float g[2], float hh[2])
{
    ax[0] = ax[1] = -1;
    float lv[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    for (int b = 0; b < 2; b++)
        for (int a = 0; a < 2 && ax[b] < 0; a++) {
            float v[2] = {0.f, 0.f}; bool have[2] = {false, false}, ok = true;
            for (int s = 0; s < 4 && ok; s++) {
                const int bit = (s >> b) & 1; const float c = cs[2 * s + a];
                if (!have[bit]) { v[bit] = c; have[bit] = true; } else if (fabsf(v[bit] - c) > 1e-6f) ok = false;
            }
            if (ok && fabsf(v[0] - v[1]) > 1e-3f) { ax[b] = a; lv[b][0] = v[0]; lv[b][1] = v[1]; }
        }
    if (ax[0] < 0 || ax[1] < 0 || ax[0] == ax[1]) return false;
    for (int b = 0; b < 2; b++) { g[b] = 2.0f * (lv[b][0] - lv[b][1]); hh[b] = lv[b][1] * lv[b][1] - lv[b][0] * lv[b][0]; }
    return true;
}

}  // namespace dvbs2
