// The held Gardner loop (the reference's `--stm-type ULTRA`): one wave per stream, lanes across the samples of a hold block.
//
// Synchronizer_Gardner_ultra_osf2::_synchronize (src/common/Module/Synchronizer/Synchronizer_timing/Synchronizer_Gardner_ultra_osf2.cpp:59-133, .hxx:58-120), restated:
//   a CONTROL sample is the whole loop: the Farrow step y = (b0 x[n-3] + b1 x[n-2]) + (b2 x[n-1] + b3 x[n]) with the taps of mu (k_timing.hip), B = is_strobe, then with
//   h = 2 prev + is_strobe (prev: the is_strobe the detector saw last)
//       the detector : h == 1: e = T1 . (T0 - y), else e = 0;  h == 1 or 2: the buffer {T0, T1} shifts in y;  h == 3: T0 = 0, T1 = y;  h == 0: nothing
//       the filter   : vi = lf_prev_in + e ki, lf_prev_in = vi, lf_output = e kp + vi
//       the control  : W = lf_output + 1/2, is_strobe = NCO < W; a strobe sets mu = NCO / W and NCO = (NCO + 1) - W, otherwise NCO -= W; the taps follow mu
//   With `act` clear every sample is a control sample.  With `act` set a frame of N samples is N / H hold blocks of H samples (blocks start over at every frame) and a tail of
//   N mod H control samples; a block is H - 4 HELD samples and four control samples.  Over the held samples mu and the taps stay, the strobe alternates from is_strobe, the
//   detector and the filter run, and NCO += is_strobe' - 1/2 with the toggled strobe.
// What a hold block leaves serial is little.  From the second held sample on the histories alternate 1, 2, so the detector's buffer holds the two outputs before the sample:
// the Farrow outputs, B and the errors of the held samples are data-parallel (lanes take samples lane, lane + 64, ...; samples 0 and 1 take the carried buffer through whatever
// history sample 0 has).  In order remain: the integrator's sum over the strobes (every other sample: 32 dependent additions per 64 samples, the addends read lane by lane), the
// NCO's half steps (a pair of them maps the NCO to itself as soon as it has done so once, which ends that walk early), lf_output of the last held sample, and the four
// control samples, which every lane of the wave computes alike.  The Farrow inputs come straight from X (the samples before the call from the state): no history is carried in
// registers, and nothing goes through LDS.  Bit for bit the CPU twin (tests/timing_ultra_twin.c); tests/timing_ultra_ref.py restates this decomposition in NumPy.
#include "dvbs2hip_internal.h"

namespace dvbs2 {

constexpr int STU_WAVES = 4;                 // streams (waves) per workgroup; the waves never meet
constexpr int STU_CTL = 61;                  // control samples per pass: their inputs and the three before them fill the 64 lanes

__device__ __forceinline__ void stu_taps(float mu, float &b0, float &b1, float &b2)
{
    const float half_mu = 0.5f * mu;
    const float half_mu_square = half_mu * mu;
    b0 = half_mu_square - half_mu;
    b1 = 1.0f - half_mu - half_mu_square;
    b2 = mu + half_mu - half_mu_square;
}

// the value lane `l` holds, for the whole wave (l the same in every lane)
__device__ __forceinline__ float stu_lane(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), __builtin_amdgcn_readfirstlane(l)));
}

__global__ void __launch_bounds__(64 * STU_WAVES)
stm_ultra_kernel(const float2 *__restrict__ X, float2 *__restrict__ Y, int2 *__restrict__ B, float *__restrict__ MU, const StmState *__restrict__ st_in,
                 StmState *__restrict__ st_out, int S, int Fs, int N, int H, int act, float kp, float ki)
{
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * STU_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (s >= S) return;
    const long long L = (long long)Fs * N;                     // complex samples per stream in this call
    const float2 *x = X + (size_t)s * (size_t)L;
    float2 *y = Y + (size_t)s * (size_t)L;
    int2 *b = B + (size_t)s * (size_t)L;
    const StmState st0 = st_in[s];
    // input sample p of the stream's run, p in [-3, L): the three before the call are the state's
    auto xin = [&](long long p) {
        if (p >= 0) return x[p];
        return p == -1 ? make_float2(st0.h[0], st0.h[1]) : p == -2 ? make_float2(st0.h[2], st0.h[3]) : make_float2(st0.h[4], st0.h[5]);
    };
    float t0r = st0.ted[0], t0i = st0.ted[1], t1r = st0.ted[2], t1i = st0.ted[3];
    float mu = st0.mu, nco = st0.nco, lfp = st0.lf_prev_in, lfo = st0.lf_output;
    int is = st0.is_strobe, prev = st0.prev_is_strobe;
    float b0, b1, b2;
    stu_taps(mu, b0, b1, b2);
    const int nb = act ? N / H : 0;                             // hold blocks per frame
    const int n = H - 4;                                        // held samples per block

    for (int f = 0; f < Fs; f++) {
        for (int blk = 0; blk <= nb; blk++) {
            long long p0 = (long long)f * N + (long long)blk * H;
            if (blk < nb) {
                // ---------------------------------------------------------------- the held samples
                const int is0 = __builtin_amdgcn_readfirstlane(is), hist0 = __builtin_amdgcn_readfirstlane(2 * prev + is);
                const int q = is0 ? 0 : 1;                                      // the strobes are the held samples q, q + 2, ...
                float a0r = t0r, a0i = t0i, a1r = t1r, a1i = t1i;               // the detector's buffer behind held sample 0
                float py1r = 0.f, py1i = 0.f, py2r = 0.f, py2i = 0.f;           // the last two outputs of the pass before
                float e_last = 0.f, yn1r = 0.f, yn1i = 0.f, yn2r = 0.f, yn2i = 0.f, y1r = 0.f, y1i = 0.f;
                for (int c = 0; c < n; c += 64) {
                    const int j = c + lane;
                    const bool ok = j < n;
                    float2 x0 = make_float2(0.f, 0.f), x1 = x0, x2 = x0, x3 = x0;
                    if (ok) { x3 = xin(p0 + j - 3); x2 = xin(p0 + j - 2); x1 = xin(p0 + j - 1); x0 = xin(p0 + j); }
                    const float yr = (b0 * x3.x + b1 * x2.x) + (b2 * x1.x + b0 * x0.x);
                    const float yi = (b0 * x3.y + b1 * x2.y) + (b2 * x1.y + b0 * x0.y);
                    const int isj = is0 ^ (j & 1);
                    if (ok) { y[p0 + j] = make_float2(yr, yi); b[p0 + j] = make_int2(isj, isj); }
                    const float u1r = __shfl_up(yr, 1), u1i = __shfl_up(yi, 1), u2r = __shfl_up(yr, 2), u2i = __shfl_up(yi, 2);
                    const float f0r = stu_lane(yr, 0), f0i = stu_lane(yi, 0);
                    // the buffer in front of lanes 0 and 1: {A0, A1} and {B0, B1}
                    float A0r, A0i, A1r, A1i, B0r, B0i, B1r, B1i;
                    if (c == 0) {
                        A0r = t0r; A0i = t0i; A1r = t1r; A1i = t1i;
                        if (hist0 == 1 || hist0 == 2) { a0r = t1r; a0i = t1i; a1r = f0r; a1i = f0i; }
                        else if (hist0 == 3) { a0r = 0.f; a0i = 0.f; a1r = f0r; a1i = f0i; }
                        B0r = a0r; B0i = a0i; B1r = a1r; B1i = a1i;
                    } else {
                        A0r = py2r; A0i = py2i; A1r = py1r; A1i = py1i;
                        B0r = py1r; B0i = py1i; B1r = f0r; B1i = f0i;
                    }
                    const float T0r = lane == 0 ? A0r : lane == 1 ? B0r : u2r, T0i = lane == 0 ? A0i : lane == 1 ? B0i : u2i;
                    const float T1r = lane == 0 ? A1r : lane == 1 ? B1r : u1r, T1i = lane == 0 ? A1i : lane == 1 ? B1i : u1i;
                    const bool used = ok && (j == 0 ? hist0 == 1 : isj == 1);   // history 1: every strobe from sample 1 on, sample 0 when the carried history says so
                    const float e = used ? T1r * (T0r - yr) + T1i * (T0i - yi) : 0.0f;
                    const float p = ok ? e * ki : -0.0f;                        // past the block's end: the addend that changes nothing
                    // the integrator, in order over the strobes
#pragma unroll
                    for (int k = 0; k < 32; k++) lfp = lfp + stu_lane(p, q + 2 * k);
                    if (c + 64 >= n) {
                        const int cnt = n - c;
                        e_last = stu_lane(e, cnt - 1);
                        yn1r = stu_lane(yr, cnt - 1); yn1i = stu_lane(yi, cnt - 1);
                        yn2r = cnt >= 2 ? stu_lane(yr, cnt - 2) : py1r; yn2i = cnt >= 2 ? stu_lane(yi, cnt - 2) : py1i;
                    }
                    if (c == 0) { y1r = stu_lane(yr, 1); y1i = stu_lane(yi, 1); }
                    py2r = stu_lane(yr, 62); py2i = stu_lane(yi, 62); py1r = stu_lane(yr, 63); py1i = stu_lane(yi, 63);
                }
                lfo = e_last * kp + lfp;
                // the detector's buffer behind the block
                if (n >= 3) { t0r = yn2r; t0i = yn2i; t1r = yn1r; t1i = yn1i; }
                else {
                    t0r = a0r; t0i = a0i; t1r = a1r; t1i = a1i;
                    if (n == 2) { t0r = t1r; t0i = t1i; t1r = y1r; t1i = y1i; }
                }
                // the NCO's n half steps, d and -d in turn: once a pair has left it as it was, every later pair does
                const float d = is0 ? -0.5f : 0.5f;
                for (int j = 0; j + 1 < n; j += 2) {
                    const float two = (nco + d) - d;
                    const bool same = __float_as_uint(two) == __float_as_uint(nco);
                    nco = two;
                    if (same) break;
                }
                if (n & 1) nco = nco + d;
                prev = is0 ^ ((n - 1) & 1);
                is = 1 - prev;
                p0 += n;
            }
            // -------------------------------------------------------------------- control samples: a block's four, or the frame's tail
            const int count = blk < nb ? 4 : N - nb * H;
            for (int c0 = 0; c0 < count; c0 += STU_CTL) {
                const int cnt = count - c0 < STU_CTL ? count - c0 : STU_CTL;
                const long long q0 = p0 + c0;
                float2 v = make_float2(0.f, 0.f);
                if (lane < cnt + 3) v = xin(q0 - 3 + lane);
                float h3r = stu_lane(v.x, 0), h3i = stu_lane(v.y, 0), h2r = stu_lane(v.x, 1), h2i = stu_lane(v.y, 1), h1r = stu_lane(v.x, 2), h1i = stu_lane(v.y, 2);
                float oyr = 0.f, oyi = 0.f;
                int ob = 0;
                for (int i = 0; i < cnt; i++) {
                    const float xr = stu_lane(v.x, i + 3), xi = stu_lane(v.y, i + 3);
                    const float yr = (b0 * h3r + b1 * h2r) + (b2 * h1r + b0 * xr);
                    const float yi = (b0 * h3i + b1 * h2i) + (b2 * h1i + b0 * xi);
                    h3r = h2r; h3i = h2i; h2r = h1r; h2i = h1i; h1r = xr; h1i = xi;
                    const int hist = 2 * prev + is;
                    if (lane == i) { oyr = yr; oyi = yi; ob = is; }
                    prev = is;
                    float e = 0.0f;
                    if (hist == 1) e = t1r * (t0r - yr) + t1i * (t0i - yi);
                    if (hist == 1 || hist == 2) { t0r = t1r; t0i = t1i; t1r = yr; t1i = yi; }
                    else if (hist == 3) { t0r = 0.f; t0i = 0.f; t1r = yr; t1i = yi; }
                    const float vi = lfp + e * ki;
                    lfp = vi;
                    lfo = e * kp + vi;
                    const float W = lfo + 0.5f;
                    is = nco < W ? 1 : 0;
                    if (is) {
                        mu = nco / W;
                        nco = nco + 1.0f;
                    }
                    nco = nco - W;
                    stu_taps(mu, b0, b1, b2);
                }
                if (lane < cnt) { y[q0 + lane] = make_float2(oyr, oyi); b[q0 + lane] = make_int2(ob, ob); }
            }
        }
        if (lane == 0) MU[(size_t)s * Fs + f] = mu;
    }
    if (lane == 0) {
        StmState st = st0;
        const float2 g1 = xin(L - 1), g2 = xin(L - 2), g3 = xin(L - 3);
        st.h[0] = g1.x; st.h[1] = g1.y; st.h[2] = g2.x; st.h[3] = g2.y; st.h[4] = g3.x; st.h[5] = g3.y;
        st.ted[0] = t0r; st.ted[1] = t0i; st.ted[2] = t1r; st.ted[3] = t1i;
        st.mu = mu; st.nco = nco; st.lf_prev_in = lfp; st.lf_output = lfo;
        st.is_strobe = is; st.prev_is_strobe = prev;
        st_out[s] = st;
    }
}

hipError_t stm_ultra_launch(const float *X, float *Y, int32_t *B, float *MU, const StmState *st_in, StmState *st_out, int S, int Fs, int N, int H, int act, float kp, float ki,
                            hipStream_t s)
{
    hipLaunchKernelGGL(stm_ultra_kernel, dim3((unsigned)((S + STU_WAVES - 1) / STU_WAVES)), dim3(64 * STU_WAVES), 0, s, reinterpret_cast<const float2 *>(X),
                       reinterpret_cast<float2 *>(Y), reinterpret_cast<int2 *>(B), MU, st_in, st_out, S, Fs, N, H, act, kp, ki);
    return hipGetLastError();
}

}  // namespace dvbs2
