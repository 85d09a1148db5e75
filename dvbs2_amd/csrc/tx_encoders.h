// The arithmetic of the two TX encoders as device functions: the BCH division and the LDPC parity rows, once, for the fused TX mirror (k_tx.hip: packed bits in,
// packed bits out) and for the task-boundary kernels (k_tx_tasks.hip: one int32 per bit in the sockets).  What differs between the two is how the bits arrive and leave,
// and that stays with the kernels.  tests/test_tx_gpu.py and tests/test_tx_tasks_gpu.py hold both forms to the same oracle and to each other.
// Device code, and tx_ldpc_lds_bytes, the launchers' size of the LDS that tx_ldpc_lds lays out.
#pragma once
#include "dvbs2hip_internal.h"

namespace dvbs2 {

// ---------------------------------------------------------------- BCH parity (Encoder_BCH_DVBS2.cpp:28-43)
// The systematic encoder is a polynomial division: parity = (u(x) x^r) mod g(x), serial along the frame.  The division is
// linear, so the frame is cut into TX_BCH_SEG consecutive segments, one LANE each (a frame per 16 lanes): the lane divides
// its segment a byte per step through a 256-entry table of (v(x) x^r) mod g(x) held in LDS (r = N - K <= 192 parity bits
// in three 64-bit words), moves its remainder to the segment's place -- times x^(8 * bytes behind the segment) mod g, a
// linear map applied bit by bit from a host-made table of x^(b + 8 after_s) mod g -- and the 16 remainders are XORed.
// (One lane per whole frame, the first version, left 4096 lanes with 7184 dependent steps each: 0.90 ms of the 2.36 ms TX.)
// One wave of 64 lanes = 64 / TX_BCH_SEG frames; T and brev are the workgroup's LDS tables.  The message is read from the packed frame p.bch_cw, which this
// function only reads.  Behind the butterfly every lane of frame f holds the whole remainder (s0, s1, s2: coefficient of x^d at bit d); live: the frame exists.
struct TxBchRem { unsigned long long s0, s1, s2; int seg, f; bool live; };
__device__ __forceinline__ TxBchRem tx_bch_remainder(const TxKParams &p, unsigned long long (*T)[3], uint8_t *brev)
{
    for (int i = threadIdx.x; i < 256; i += 64) {
        T[i][0] = p.bch_tab[3 * i]; T[i][1] = p.bch_tab[3 * i + 1]; T[i][2] = p.bch_tab[3 * i + 2];
        uint32_t r = 0; for (int b = 0; b < 8; b++) if (i >> b & 1) r |= 1u << (7 - b);
        brev[i] = (uint8_t)r;
    }
    __syncthreads();
    const int seg = threadIdx.x & (TX_BCH_SEG - 1);
    const int f = blockIdx.x * (64 / TX_BCH_SEG) + (threadIdx.x / TX_BCH_SEG);
    const bool live = f < p.n_frames;
    const int K = p.K_bch, r = p.K_ldpc - p.K_bch;
    const int nw_out = (p.K_ldpc + 31) / 32;
    const uint32_t *cw = p.bch_cw + (size_t)(live ? f : 0) * nw_out;
    unsigned long long s0 = 0, s1 = 0, s2 = 0;
    const int tw = (r - 8) >> 6, ts = (r - 8) & 63;            // where the top byte of the remainder sits
    const unsigned long long m1 = r >= 128 ? ~0ull : r > 64 ? (1ull << (r - 64)) - 1ull : 0ull;
    const unsigned long long m2 = r >= 192 ? ~0ull : r > 128 ? (1ull << (r - 128)) - 1ull : 0ull;
    const int nbytes = K / 8, L = (nbytes + TX_BCH_SEG - 1) / TX_BCH_SEG;
    const int b0 = min(seg * L, nbytes), b1 = min(b0 + L, nbytes);
    if (live && b1 > b0) {
        // the message words of the segment, 8 at a time and one batch ahead: the division is a dependent chain (table look-up
        // -> XOR -> next look-up) and must not also wait for a global load every four bytes
        constexpr int WB = 8;
        const int w0 = b0 >> 2, w1 = (b1 - 1) >> 2;           // first / last word touched
        uint32_t nxt[WB];
#pragma unroll
        for (int k = 0; k < WB; k++) nxt[k] = cw[min(w0 + k, w1)];
        for (int wb = w0; wb <= w1; wb += WB) {
            uint32_t cur[WB];
#pragma unroll
            for (int k = 0; k < WB; k++) cur[k] = nxt[k];
#pragma unroll
            for (int k = 0; k < WB; k++) nxt[k] = cw[min(wb + WB + k, w1)];
#pragma unroll
            for (int k = 0; k < WB; k++) {
#pragma unroll
                for (int bb = 0; bb < 4; bb++) {
                    const int by = 4 * (wb + k) + bb;
                    if (by < b0 || by >= b1) continue;
                    const uint32_t raw = (cur[k] >> (bb * 8)) & 0xFFu;
                    const uint32_t top = (uint32_t)((tw == 0 ? s0 : tw == 1 ? s1 : s2) >> ts) & 0xFFu;
                    const uint32_t idx = top ^ brev[raw];
                    s2 = ((s2 << 8) | (s1 >> 56)) & m2; s1 = ((s1 << 8) | (s0 >> 56)) & m1; s0 <<= 8;
                    if (r <= 64) s0 &= (r == 64 ? ~0ull : (1ull << r) - 1ull);
                    s0 ^= T[idx][0]; s1 ^= T[idx][1]; s2 ^= T[idx][2];
                }
            }
        }
    }
    // to the segment's place: sum over the set bits b of the remainder of x^(b + 8 (nbytes - b1)) mod g
    if (b1 < nbytes) {
        const unsigned long long *P = p.bch_shift + (size_t)seg * r * 3;
        unsigned long long a0 = 0, a1 = 0, a2 = 0;
        for (int b0 = 0; b0 < r; b0 += 8) {               // r is a multiple of 8 (m t, m = 14 or 16); 24 table loads in flight
            unsigned long long q0[8], q1[8], q2[8];
#pragma unroll
            for (int k = 0; k < 8; k++) { q0[k] = P[3 * (b0 + k)]; q1[k] = P[3 * (b0 + k) + 1]; q2[k] = P[3 * (b0 + k) + 2]; }
            const unsigned long long sw = b0 < 64 ? s0 >> b0 : b0 < 128 ? s1 >> (b0 - 64) : s2 >> (b0 - 128);      // 8 bits of the remainder (b0 is a multiple of 8)
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const unsigned long long m = 0ull - ((sw >> k) & 1ull);
                a0 ^= q0[k] & m; a1 ^= q1[k] & m; a2 ^= q2[k] & m;
            }
        }
        s0 = a0; s1 = a1; s2 = a2;
    }
    for (int o = TX_BCH_SEG / 2; o > 0; o >>= 1) { s0 ^= __shfl_xor(s0, o); s1 ^= __shfl_xor(s1, o); s2 ^= __shfl_xor(s2, o); }
    return TxBchRem{s0, s1, s2, seg, f, live};
}
// parity bit j of r (coefficient of x^(r-1) first, DVB-S2 order)
__device__ __forceinline__ uint32_t tx_bch_parity_bit(const TxBchRem &R, int r, int j)
{
    const int d = r - 1 - j;
    return d < 64 ? (uint32_t)(R.s0 >> d) & 1u : d < 128 ? (uint32_t)(R.s1 >> (d - 64)) & 1u : (uint32_t)(R.s2 >> (d - 128)) & 1u;
}

// ---------------------------------------------------------------- LDPC IRA encoder (ETSI EN 302 307 5.3.2)
// One workgroup per frame.  parity accumulator address (a + m q) mod M <=> check (r, t): the same circulant structure the decoder
// uses, i.e. accumulator row r (its 360 bits t) = XOR over the row's edges (bit-group g, shift t0) of bit-group g ROTATED by t0.
// Rows are 12 packed words: a lane forms one word of one row, an edge costs it two funnel shifts out of the packed info bits (the
// wrap of the 360-bit circle splits a window in two) instead of 32 single-bit gathers -- 1 / 16 of the instructions of one lane per check.
// Then p_c ^= p_{c-1} over c = q t + r: a running XOR of the rows (prefix over r inside a column) and an exclusive prefix over t of
// the column totals, both on packed words.
constexpr int ENC_W = (LDPC_Z + 31) / 32;                            // 12 words per 360-bit row, the last one holds 8 bits
__device__ __forceinline__ uint32_t enc_window(const uint32_t *info, int pos)      // 32 bits of the packed info from bit `pos` on
{
    return __funnelshift_r(info[pos >> 5], info[(pos >> 5) + 1], pos & 31);
}
struct TxLdpcLds {
    uint32_t *info;          // nw_in words + one of padding (a window may start in the last word)
    uint32_t *prow;          // [r][ENC_W] packed parity rows
    uint32_t *excl;          // ENC_W words: exclusive prefix over t of the column totals
    uint32_t *tab;           // the layer table (t0 | group << 9 per entry): no global round trip per entry
};
__device__ __forceinline__ TxLdpcLds tx_ldpc_lds(uint32_t *sm, const TxKParams &p)
{
    const int q = (p.N_ldpc - p.K_ldpc) / LDPC_Z, nw_in = (p.K_ldpc + 31) / 32;
    TxLdpcLds s;
    s.info = sm; s.prow = sm + nw_in + 1; s.excl = s.prow + q * ENC_W; s.tab = s.excl + ENC_W;
    return s;
}
inline size_t tx_ldpc_lds_bytes(const TxKParams &p)                  // info (+1) | rows | prefix | table
{
    const size_t q_enc = (size_t)((p.N_ldpc - p.K_ldpc) / LDPC_Z);
    return ((size_t)((p.K_ldpc + 31) / 32) + 1 + (q_enc + 1) * ENC_W + q_enc * p.enc_stride) * 4;
}
// from the packed info bits in s.info and the table in s.tab (both complete: the caller has synchronised) to the parity rows and the column prefix;
// the caller synchronises again before it reads them
__device__ __forceinline__ void tx_ldpc_rows(const TxKParams &p, const TxLdpcLds &s, int t)
{
    const int q = (p.N_ldpc - p.K_ldpc) / LDPC_Z;
    const uint32_t *info = s.info;
    uint32_t *prow = s.prow, *excl = s.excl;
    for (int task = t; task < q * ENC_W; task += LDPC_THREADS) {
        const int r = task / ENC_W, l = task - r * ENC_W;
        const int deg = p.enc_deg[r];
        const uint32_t *T = s.tab + r * p.enc_stride;
        uint32_t acc = 0u;
#pragma unroll 4
        for (int j = 0; j < deg; j++) {
            const uint32_t e = T[j];                                  // t0 | group << 9
            int m0 = 32 * l - (int)(e & 0x1FFu); m0 += m0 < 0 ? LDPC_Z : 0;      // source index of the word's first bit: (32 l - t0) mod 360
            const int base = (int)(e >> 9) * LDPC_Z, n1 = LDPC_Z - m0;              // n1 bits are left before the circle wraps
            uint32_t w = enc_window(info, base + m0);
            if (n1 < 32) w = (w & ((1u << n1) - 1u)) | (enc_window(info, base) << n1);
            acc ^= w;
        }
        prow[task] = l == ENC_W - 1 ? acc & ((1u << (LDPC_Z - 32 * (ENC_W - 1))) - 1u) : acc;
    }
    __syncthreads();
    if (t < ENC_W) {
        // prefix over r inside every column (12 lanes, one word of every row each), then the exclusive prefix over t of the column totals
        uint32_t x = 0u;
        for (int r = 0; r < q; r++) { x ^= prow[r * ENC_W + t]; prow[r * ENC_W + t] = x; }
        uint32_t incl = x;
        incl ^= incl << 1; incl ^= incl << 2; incl ^= incl << 4; incl ^= incl << 8; incl ^= incl << 16;      // inclusive prefix XOR inside the word
        uint32_t par = incl >> 31;                                    // parity of the whole word (full words only matter: the last one has no successor)
        uint32_t carry = 0u;
        for (int l = 0; l < ENC_W; l++) { const uint32_t pl = (uint32_t)__shfl((int)par, l); if (l < t) carry ^= pl; }
        excl[t] = (incl << 1) ^ (carry ? 0xFFFFFFFFu : 0u);
    }
}
// parity bit c = q tt + r
__device__ __forceinline__ uint32_t tx_ldpc_parity_bit(const TxLdpcLds &s, int r, int tt)
{
    return ((s.prow[r * ENC_W + (tt >> 5)] ^ s.excl[tt >> 5]) >> (tt & 31)) & 1u;
}

}  // namespace dvbs2
