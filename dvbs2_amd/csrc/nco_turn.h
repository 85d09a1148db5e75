/* cos and sin of a whole number of millionths of a turn, in fp32, written out: no library routine, no fused operation (every translation unit that includes this is
 * compiled with -ffp-contract=off), so that a host compiler and hipcc give the same bits.  Plain C; included by k_stepmf.hip and by tests/stepmf_twin.c.
 *
 * Why millionths: Multiplier_sine_ccc_naive keeps nu to six decimals (set_nu, Multiplier_sine_ccc_naive.cpp:44-51) and counts n = 0 .. 999999 (step, :69-75), so the
 * phase nu n is (k n mod 1e6) / 1e6 turns with k = nu 1e6 a whole number: exact in integers.  The reference evaluates cos / sin of the fp32 product omega n instead,
 * whose rounding alone is up to 2^-24 omega n (0.2 rad at omega n = 3e6); this form is the more accurate one.
 *
 * The octant comes off in integers, the argument left is x in [0, pi/4], and sin x / cos x are their Taylor polynomials to x^9 / x^8 in Horner form (truncation 1.7e-9 /
 * 2.5e-8).  Worst error against double-precision cos / sin over all 1e6 arguments: tests/test_stepmf_twin.py measures and asserts it (9.3e-8; the bar is 2e-6). */
#ifndef DVBS2_NCO_TURN_H
#define DVBS2_NCO_TURN_H

#if defined(__HIPCC__)
#define NCO_TURN_FN __host__ __device__ static inline
#else
#define NCO_TURN_FN static inline
#endif

#define NCO_TURN_UNITS 1000000          /* p counts turns / 1e6 */

/* (k n) mod 1e6 for a frequency of k millionths of a cycle per sample (any sign) at sample n in [0, 1e6) */
NCO_TURN_FN int nco_turn_index(int k, int n)
{
    int km = k % NCO_TURN_UNITS;
    if (km < 0) km += NCO_TURN_UNITS;
    return (int)(((long long)km * (long long)n) % NCO_TURN_UNITS);
}

/* p in [0, 1e6): *c = cos(2 pi p / 1e6), *s = sin(2 pi p / 1e6) */
NCO_TURN_FN void nco_turn_cs(int p, float *c, float *s)
{
    const int oct = p / 125000;
    int r = p - oct * 125000;
    if (oct & 1) r = 125000 - r;                           /* odd octants run backwards: x stays in [0, pi/4] */
    const float x = (float)r * 6.2831853071795865e-6f;     /* r < 2^24: exact; one rounding of the constant, one of the product */
    const float x2 = x * x;
    float ps = x2 * 2.7557319223985893e-6f;                /* sin x = x (1 - x2/6 + x2^2/120 - x2^3/5040 + x2^4/362880) */
    ps = x2 * (ps - 1.9841269841269841e-4f);
    ps = x2 * (ps + 8.3333333333333333e-3f);
    ps = x2 * (ps - 1.6666666666666667e-1f);
    ps = x * (ps + 1.0f);
    float pc = x2 * 2.4801587301587302e-5f;                /* cos x = 1 - x2/2 + x2^2/24 - x2^3/720 + x2^4/40320 */
    pc = x2 * (pc - 1.3888888888888889e-3f);
    pc = x2 * (pc + 4.1666666666666667e-2f);
    pc = x2 * (pc - 0.5f);
    pc = pc + 1.0f;
    const int swap = ((oct + 1) >> 1) & 1;                 /* octants 1, 2, 5, 6: the angle is a quarter turn -+ x */
    const float ac = swap ? ps : pc, as = swap ? pc : ps;
    *c = (oct >= 2 && oct <= 5) ? -ac : ac;
    *s = oct >= 4 ? -as : as;
}

#endif
