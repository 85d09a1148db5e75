// Symbol-timing recovery (the reference's `--stm-type FAST` synchronizer, Gardner's detector at two samples per symbol) and the channel's delay tasks.
//
// stm_sync_kernel is Synchronizer_Gardner_fast_osf2::_synchronize (src/common/Module/Synchronizer/Synchronizer_timing/Synchronizer_Gardner_fast_osf2.cpp:35-166): per input sample the
// Farrow step and gardner_synchronize of gardner_loop.h, which states the loop.  B is written for both reals of the sample (the int socket B_N1), MU per frame is mu after the
// frame (Synchronizer_timing.hxx:189-201).  The loop is sample-serial within a stream.
// Across streams it is not: one lane per stream, a wave carries 64 streams.  The frames of a call are stream-major (stream s = frames [s F/S, (s+1) F/S)), so a lane's samples
// are one contiguous run and the 64 runs of a wave lie a stream apart; tiles of 64 samples of the 64 streams go through LDS (coalesced row loads, a lane-private walk over its own
// row, the outputs written back into the same slots, coalesced row stores).  The tile's loads and the LDS reads do not depend on the chain.
//
// Synchronizer_timing::_extract (Synchronizer_timing.hxx:262-304): the strobed reals of the stream, after what the carry buffer held, fill the N_out * F/S reals of Y_N2; what
// overflows goes to the carry buffer for the next call.  Too few (an underflow): everything stays in the carry buffer, the frame the output would have reached counts an
// underflow and the stream is reported not ready (the reference throws processing_aborted there).  One workgroup per stream, a block-wide prefix count over B_N1.
//
// The channel's delay tasks (src/common/Factory/DVBS2/DVBS2.cpp:520-544, bound frame delay -> integer delay -> fractional delay in CH/main.cpp:60-62): the frame delay
// (Filter_buffered_delay, (floor(D) - 2) / N frames) and the integer delay (Variable_delay_cc_naive, (floor(D) - 2) mod N samples) are zero-initialised delay lines whose
// composition is one delay line of floor(D) - 2 samples; the fractional delay is the same Farrow interpolator with mu = D - floor(D) fixed.  Data-parallel: a thread per sample,
// floor(D) + 1 samples of history kept between calls.
#include "gardner_loop.h"

namespace dvbs2 {

constexpr int STM_T = 64;                    // samples per stream and tile
constexpr int STM_ROW = 2 * STM_T + 1;       // floats per LDS row: odd, so that the 64 lanes' walks hit 64 different banks
constexpr int STM_FROW = STM_T + 1;          // strobe flags per LDS row
constexpr int STM_EX_THREADS = 256;

__global__ void __launch_bounds__(64)
stm_sync_kernel(const float2 *__restrict__ X, float2 *__restrict__ Y, int2 *__restrict__ B, float *__restrict__ MU, const StmState *__restrict__ st_in,
                StmState *__restrict__ st_out, int S, int Fs, int N, float kp, float ki)
{
    __shared__ float tile[64 * STM_ROW];
    __shared__ int flg[64 * STM_FROW];
    const int lane = threadIdx.x;
    const int s0 = blockIdx.x * 64;
    const int rows = S - s0 < 64 ? S - s0 : 64;
    const int s = s0 + lane;
    const bool act = lane < rows;
    const long long L = (long long)Fs * N;                     // complex samples per stream in this call

    StmState st = {};
    if (act) st = st_in[s];
    GardnerRegs g;
    g.load(st);
    int to_frame_end = N;                                       // samples left in the current frame
    int frame = 0;
    float *row = tile + lane * STM_ROW;
    int *frow = flg + lane * STM_FROW;

    for (long long t0 = 0; t0 < L; t0 += STM_T) {
        const int cnt = L - t0 < STM_T ? (int)(L - t0) : STM_T;
        if (lane < cnt) {
#pragma unroll 8
            for (int r = 0; r < rows; r++) {
                const float2 v = X[(size_t)(s0 + r) * (size_t)L + (size_t)t0 + lane];
                tile[r * STM_ROW + 2 * lane] = v.x;
                tile[r * STM_ROW + 2 * lane + 1] = v.y;
            }
        }
        __syncthreads();
        if (act) {
            for (int i = 0; i < cnt; i++) {
                float yr, yi;
                g.farrow(row[2 * i], row[2 * i + 1], yr, yi);
                const int strobe = gardner_synchronize(g, yr, yi, kp, ki);
                row[2 * i] = yr;
                row[2 * i + 1] = yi;
                frow[i] = strobe;
                if (--to_frame_end == 0) {
                    MU[(size_t)s * Fs + frame] = g.mu;
                    frame++;
                    to_frame_end = N;
                }
            }
        }
        __syncthreads();
        if (lane < cnt) {
#pragma unroll 8
            for (int r = 0; r < rows; r++) {
                const size_t o = (size_t)(s0 + r) * (size_t)L + (size_t)t0 + lane;
                Y[o] = make_float2(tile[r * STM_ROW + 2 * lane], tile[r * STM_ROW + 2 * lane + 1]);
                const int f = flg[r * STM_FROW + lane];
                B[o] = make_int2(f, f);
            }
        }
        __syncthreads();
    }
    if (act) {
        g.store(st);
        st_out[s] = st;
    }
}

// exclusive prefix sum of v over the workgroup (STM_EX_THREADS lanes); *total = the sum
__device__ __forceinline__ int block_exclusive_scan(int v, int *wsum, int *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < STM_EX_THREADS / 64; k++) {
        const int t = wsum[k];
        before += k < w ? t : 0;
        all += t;
    }
    __syncthreads();                     // wsum is reused by the next call
    *total = all;
    return before + inc - v;
}

__global__ void __launch_bounds__(STM_EX_THREADS)
stm_extract_kernel(const float2 *__restrict__ Y1, const int2 *__restrict__ B1, float *__restrict__ Y2, int32_t *__restrict__ UFW, int32_t *__restrict__ RDY,
                   const float *__restrict__ c_in, const int32_t *__restrict__ n_in, float *__restrict__ c_out, int32_t *__restrict__ n_out, int32_t *__restrict__ uf,
                   int Fs, int N, long long cap)
{
    __shared__ int wsum[STM_EX_THREADS / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    const long long L = (long long)Fs * N;          // complex samples of the stream in this call
    const long long M = (long long)Fs * N;          // reals of Y_N2 for the stream: N_out = N_in / osf = N reals per frame
    const float *ci = c_in + (size_t)s * cap;
    float *co = c_out + (size_t)s * cap;
    float *y2 = Y2 + (size_t)s * M;
    const float2 *y1 = Y1 + (size_t)s * L;
    const int2 *b1 = B1 + (size_t)s * L;
    const long long head = n_in[s];
    const long long tmp = head < M ? head : M;
    for (long long k = tid; k < tmp; k += STM_EX_THREADS) y2[k] = ci[k];
    for (long long k = tid; k < head - tmp; k += STM_EX_THREADS) co[k] = ci[tmp + k];
    const long long ovf = head - tmp - M;           // carry slot of output position p >= M: ovf + p
    long long n = tmp;
    for (long long i0 = 0; i0 < L; i0 += STM_EX_THREADS) {
        const long long i = i0 + tid;
        int2 b = make_int2(0, 0);
        float2 v = make_float2(0.f, 0.f);
        if (i < L) { b = b1[i]; v = y1[i]; }
        const int c = (b.x != 0) + (b.y != 0);
        int total;
        long long p = n + block_exclusive_scan(c, wsum, &total);
        if (b.x) { if (p < M) y2[p] = v.x; else if (ovf + p < cap) co[ovf + p] = v.x; p++; }
        if (b.y) { if (p < M) y2[p] = v.y; else if (ovf + p < cap) co[ovf + p] = v.y; }
        n += total;
    }
    const bool ready = n >= M;
    if (!ready) {
        // underflow: head <= M here, so tmp = head and nothing overflowed; the carry buffer takes all n reals again, from the sources
        for (long long k = tid; k < tmp; k += STM_EX_THREADS) co[k] = ci[k];
        long long m = tmp;
        for (long long i0 = 0; i0 < L; i0 += STM_EX_THREADS) {
            const long long i = i0 + tid;
            int2 b = make_int2(0, 0);
            float2 v = make_float2(0.f, 0.f);
            if (i < L) { b = b1[i]; v = y1[i]; }
            const int c = (b.x != 0) + (b.y != 0);
            int total;
            long long p = m + block_exclusive_scan(c, wsum, &total);
            if (b.x) { if (p < cap) co[p] = v.x; p++; }
            if (b.y) { if (p < cap) co[p] = v.y; }
            m += total;
        }
    }
    if (tid == 0) {
        const long long k = ready ? ovf + n : n;
        n_out[s] = (int32_t)(k < cap ? k : cap);
        RDY[s] = ready ? (k > cap ? 2 : 1) : 0;          // 2: ready, but the carry buffer was full and lost k - cap reals
    }
    // UFW = the underflows counted since the stream's last ready call, this one's included; a ready call clears the count (Synchronizer_timing.hxx:255-259)
    const long long uframe = ready ? -1 : n / N;
    for (int f = tid; f < Fs; f += STM_EX_THREADS) {
        const size_t g = (size_t)s * Fs + f;
        const int32_t v = uf[g] + (f == uframe ? 1 : 0);
        UFW[g] = v;
        uf[g] = ready ? 0 : v;
    }
}

__global__ void __launch_bounds__(256)
chn_delay_kernel(const float2 *__restrict__ X, float2 *__restrict__ Y, const float2 *__restrict__ h_in, float2 *__restrict__ h_out, long long H, long long T,
                 float b0, float b1, float b2)
{
    // c = h_in (H samples) followed by X (T samples); y[n] = (b0 c[n] + b1 c[n+1]) + (b2 c[n+2] + b3 c[n+3]) with b3 = b0; h_out = the last H samples of c
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    auto c = [&](long long j) { return j < H ? h_in[j] : X[j - H]; };
    if (n < T) {
        const float2 c0 = c(n), c1 = c(n + 1), c2 = c(n + 2), c3 = c(n + 3);
        Y[n] = make_float2(farrow_sum(b0, b1, b2, c0.x, c1.x, c2.x, c3.x), farrow_sum(b0, b1, b2, c0.y, c1.y, c2.y, c3.y));
    }
    if (n < H) h_out[n] = c(T + n);
}

hipError_t stm_sync_launch(const float *X, float *Y, int32_t *B, float *MU, const StmState *st_in, StmState *st_out, int S, int Fs, int N, float kp, float ki, hipStream_t s)
{
    hipLaunchKernelGGL(stm_sync_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, s, reinterpret_cast<const float2 *>(X), reinterpret_cast<float2 *>(Y),
                       reinterpret_cast<int2 *>(B), MU, st_in, st_out, S, Fs, N, kp, ki);
    return hipGetLastError();
}

hipError_t stm_extract_launch(const float *Y1, const int32_t *B1, float *Y2, int32_t *UFW, int32_t *RDY, const float *c_in, const int32_t *n_in, float *c_out, int32_t *n_out,
                              int32_t *uf, int S, int Fs, int N, long long cap, hipStream_t s)
{
    hipLaunchKernelGGL(stm_extract_kernel, dim3((unsigned)S), dim3(STM_EX_THREADS), 0, s, reinterpret_cast<const float2 *>(Y1), reinterpret_cast<const int2 *>(B1), Y2, UFW, RDY,
                       c_in, n_in, c_out, n_out, uf, Fs, N, cap);
    return hipGetLastError();
}

hipError_t chn_delay_launch(const float *X, float *Y, const float *h_in, float *h_out, long long H, long long T, float b0, float b1, float b2, hipStream_t s)
{
    const long long n = T > H ? T : H;
    hipLaunchKernelGGL(chn_delay_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float2 *>(X), reinterpret_cast<float2 *>(Y),
                       reinterpret_cast<const float2 *>(h_in), reinterpret_cast<float2 *>(h_out), H, T, b0, b1, b2);
    return hipGetLastError();
}

}  // namespace dvbs2
