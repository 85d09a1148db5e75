// The held Gardner loop (the reference's `--stm-type ULTRA`): one wave per stream, lanes across the samples of a hold block.
//
// Synchronizer_Gardner_ultra_osf2::_synchronize (src/common/Module/Synchronizer/Synchronizer_timing/Synchronizer_Gardner_ultra_osf2.cpp:59-133, .hxx:58-120), restated:
//   a CONTROL sample is the whole loop: the Farrow step with the taps of mu, B = is_strobe, then detector, loop filter and interpolation control -- gardner_ultra of
//   gardner_loop.h, which states the loop and how this form differs from FAST's two.
//   With `act` clear every sample is a control sample.  With `act` set a frame of N samples is N / H hold blocks of H samples (blocks start over at every frame) and a tail of
//   N mod H control samples; a block is H - 4 HELD samples and four control samples.  Over the held samples mu and the taps stay, the strobe alternates from is_strobe, the
//   detector and the filter run, and NCO += is_strobe' - 1/2 with the toggled strobe.
// What a hold block leaves serial is little.  From the second held sample on the histories alternate 1, 2, so the detector's buffer holds the two outputs before the sample:
// the Farrow outputs, B and the errors of the held samples are data-parallel (lanes take samples lane, lane + 64, ...; samples 0 and 1 take the carried buffer through whatever
// history sample 0 has).  In order remain: the integrator's sum over the strobes (every other sample: 32 dependent additions per 64 samples, the addends read lane by lane), the
// NCO's half steps (a pair of them maps the NCO to itself as soon as it has done so once, which ends that walk early), lf_output of the last held sample, and the four
// control samples, which every lane of the wave computes alike.  The Farrow inputs come straight from X (the samples before the call from the state): no history is carried in
// registers, and nothing goes through LDS.  Bit for bit the CPU twin (tests/timing_ultra_twin.c); tests/timing_ultra_ref.py restates this decomposition in NumPy.
#include "gardner_loop.h"

namespace dvbs2 {

constexpr int STU_WAVES = 4;                 // streams (waves) per workgroup; the waves never meet
constexpr int STU_CTL = 61;                  // control samples per pass: their inputs and the three before them fill the 64 lanes

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
    GardnerRegs g;
    g.load(st0);                                                // (its Farrow history is refilled from the inputs by every control pass)
    const int nb = act ? N / H : 0;                             // hold blocks per frame
    const int n = H - 4;                                        // held samples per block

    for (int f = 0; f < Fs; f++) {
        for (int blk = 0; blk <= nb; blk++) {
            long long p0 = (long long)f * N + (long long)blk * H;
            if (blk < nb) {
                // ---------------------------------------------------------------- the held samples
                const int is0 = __builtin_amdgcn_readfirstlane(g.is), hist0 = __builtin_amdgcn_readfirstlane(2 * g.prev + g.is);
                const int q = is0 ? 0 : 1;                                      // the strobes are the held samples q, q + 2, ...
                float a0r = g.t0r, a0i = g.t0i, a1r = g.t1r, a1i = g.t1i;       // the detector's buffer behind held sample 0
                float py1r = 0.f, py1i = 0.f, py2r = 0.f, py2i = 0.f;           // the last two outputs of the pass before
                float e_last = 0.f, yn1r = 0.f, yn1i = 0.f, yn2r = 0.f, yn2i = 0.f, y1r = 0.f, y1i = 0.f;
                for (int c = 0; c < n; c += 64) {
                    const int j = c + lane;
                    const bool ok = j < n;
                    float2 x0 = make_float2(0.f, 0.f), x1 = x0, x2 = x0, x3 = x0;
                    if (ok) { x3 = xin(p0 + j - 3); x2 = xin(p0 + j - 2); x1 = xin(p0 + j - 1); x0 = xin(p0 + j); }
                    // farrow_sum's expression, written out: through the function this kernel's register allocation changes (94 VGPRs for 92)
                    const float yr = (g.b0 * x3.x + g.b1 * x2.x) + (g.b2 * x1.x + g.b0 * x0.x);
                    const float yi = (g.b0 * x3.y + g.b1 * x2.y) + (g.b2 * x1.y + g.b0 * x0.y);
                    const int isj = is0 ^ (j & 1);
                    if (ok) { y[p0 + j] = make_float2(yr, yi); b[p0 + j] = make_int2(isj, isj); }
                    const float u1r = __shfl_up(yr, 1), u1i = __shfl_up(yi, 1), u2r = __shfl_up(yr, 2), u2i = __shfl_up(yi, 2);
                    const float f0r = stu_lane(yr, 0), f0i = stu_lane(yi, 0);
                    // the buffer in front of lanes 0 and 1: {A0, A1} and {B0, B1}
                    float A0r, A0i, A1r, A1i, B0r, B0i, B1r, B1i;
                    if (c == 0) {
                        A0r = g.t0r; A0i = g.t0i; A1r = g.t1r; A1i = g.t1i;
                        if (hist0 == 1 || hist0 == 2) { a0r = g.t1r; a0i = g.t1i; a1r = f0r; a1i = f0i; }
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
                    for (int k = 0; k < 32; k++) g.lfp = g.lfp + stu_lane(p, q + 2 * k);
                    if (c + 64 >= n) {
                        const int cnt = n - c;
                        e_last = stu_lane(e, cnt - 1);
                        yn1r = stu_lane(yr, cnt - 1); yn1i = stu_lane(yi, cnt - 1);
                        yn2r = cnt >= 2 ? stu_lane(yr, cnt - 2) : py1r; yn2i = cnt >= 2 ? stu_lane(yi, cnt - 2) : py1i;
                    }
                    if (c == 0) { y1r = stu_lane(yr, 1); y1i = stu_lane(yi, 1); }
                    py2r = stu_lane(yr, 62); py2i = stu_lane(yi, 62); py1r = stu_lane(yr, 63); py1i = stu_lane(yi, 63);
                }
                g.lfo = e_last * kp + g.lfp;
                // the detector's buffer behind the block
                if (n >= 3) { g.t0r = yn2r; g.t0i = yn2i; g.t1r = yn1r; g.t1i = yn1i; }
                else {
                    g.t0r = a0r; g.t0i = a0i; g.t1r = a1r; g.t1i = a1i;
                    if (n == 2) { g.t0r = g.t1r; g.t0i = g.t1i; g.t1r = y1r; g.t1i = y1i; }
                }
                // the NCO's n half steps, d and -d in turn: once a pair has left it as it was, every later pair does
                const float d = is0 ? -0.5f : 0.5f;
                for (int j = 0; j + 1 < n; j += 2) {
                    const float two = (g.nco + d) - d;
                    const bool same = __float_as_uint(two) == __float_as_uint(g.nco);
                    g.nco = two;
                    if (same) break;
                }
                if (n & 1) g.nco = g.nco + d;
                g.prev = is0 ^ ((n - 1) & 1);
                g.is = 1 - g.prev;
                p0 += n;
            }
            // -------------------------------------------------------------------- control samples: a block's four, or the frame's tail
            const int count = blk < nb ? 4 : N - nb * H;
            for (int c0 = 0; c0 < count; c0 += STU_CTL) {
                const int cnt = count - c0 < STU_CTL ? count - c0 : STU_CTL;
                const long long q0 = p0 + c0;
                float2 v = make_float2(0.f, 0.f);
                if (lane < cnt + 3) v = xin(q0 - 3 + lane);
                g.h3r = stu_lane(v.x, 0); g.h3i = stu_lane(v.y, 0); g.h2r = stu_lane(v.x, 1); g.h2i = stu_lane(v.y, 1); g.h1r = stu_lane(v.x, 2); g.h1i = stu_lane(v.y, 2);
                float oyr = 0.f, oyi = 0.f;
                int ob = 0;
                for (int i = 0; i < cnt; i++) {
                    float yr, yi;
                    g.farrow(stu_lane(v.x, i + 3), stu_lane(v.y, i + 3), yr, yi);
                    const int strobe = gardner_ultra(g, yr, yi, kp, ki);
                    if (lane == i) { oyr = yr; oyi = yi; ob = strobe; }
                }
                if (lane < cnt) { y[q0 + lane] = make_float2(oyr, oyi); b[q0 + lane] = make_int2(ob, ob); }
            }
        }
        if (lane == 0) MU[(size_t)s * Fs + f] = g.mu;
    }
    if (lane == 0) {
        StmState st;
        g.store(st);                                            // last_symbol as it came: this loop does not maintain it
        const float2 g1 = xin(L - 1), g2 = xin(L - 2), g3 = xin(L - 3);
        st.h[0] = g1.x; st.h[1] = g1.y; st.h[2] = g2.x; st.h[3] = g2.y; st.h[4] = g3.x; st.h[5] = g3.y;
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
