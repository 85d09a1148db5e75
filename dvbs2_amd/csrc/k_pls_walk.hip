// PLHEADER walk: the chain of PL frames of a stream whose MODCOD changes from frame to frame (VCM / ACM), from the header at `start` to the end of the buffer, and the
// frames grouped by PLS value as pointer tables for the located decoders (include/dvbs2hip.h has the definition).  An extension with no reference task.
//
// Every PL frame length is a multiple of 18 symbols, so the headers of a chain sit at the candidates c_i = start + 18 i, i < M, and the PLS decoder (k_pls.hip, at a
// stride of 18) has been run on those alone before any kernel of this file.  Node i is a frame when its length L = LEN'[PLS[i]] is not 0, q(i) >= q_min and c_i + L <=
// n_sym; every other node stops a walk that reaches it (LOST or END), and so does the end of the candidates.  A frame's successor is i + L / 18: forward only.
//   - init: level 0 of the jump table, jump[0][i] = the successor of a frame (M, "none", where it is past the candidates or i is no frame), and rank[i] = -1 but rank[0] = 0;
//   - double, level k -> k + 1: jump[k+1][i] = jump[k][jump[k][i]] -- the node 2^(k+1) frames on, or M;
//   - mark, level K - 1 down to 0: a node of rank r >= 0 gives jump[k][i] the rank r + 2^k.  A node of rank r is reached from the node of rank r minus r's lowest set
//     bit, which the levels above have marked, so after level 0 every node up to 2^K - 1 frames behind node 0 has its rank, and no other node has one.  A rank written
//     in a launch may or may not be seen by another lane of the same launch; what that lane then writes is again the true rank of a node of the chain: integers only,
//     the same result whatever the order;
//   - emit: a ranked frame of rank r < max_out writes OFF, VAL, Q at r; the one node that ends the walk -- a ranked node that is no frame, the frame of rank max_out
//     (FULL), or the frame whose successor is past the candidates (END) -- writes RES;
//   - group: one workgroup, thread v counts value v and, behind an exclusive scan of the 256 counts, writes its frames' IDX and SRC in stream order: VAL and OFF go
//     through LDS a tile at a time, every thread reads every entry as a broadcast.
// K, the number of levels, is fixed on the host from max_out and the largest number of frames M candidates can hold: no host round trip, no workgroup waits on another.
// pls_walk_lane_kernel is the same walk by one lane, one dependent load per frame: the yardstick of results/pls_walk/README.md, and what a walk of few levels runs.
#include "dvbs2hip_internal.h"

namespace dvbs2 {

namespace {

constexpr int PW_END = 0, PW_LOST = 1, PW_FULL = 2;
constexpr int PW_TILE = 2048;                    // entries of VAL and OFF a pass of the grouping holds in LDS

// node i at symbol c: value, q and hop (candidates to the successor); -1 for a frame, or the status with which a walk stops here
__device__ __forceinline__ int pw_node(const int32_t *__restrict__ PLS, const float *__restrict__ MET, const float *__restrict__ ENE, const int32_t *__restrict__ LEN,
                                       int i, int c, int n_sym, float q_min, int32_t &v, float &q, int32_t &hop)
{
    v = PLS[i] & 255;
    const float m = MET[i], e = ENE[i];
    q = e == 0.f ? 0.f : (m * m) / (90.f * e);
    int32_t L = LEN[v];
    if (L < 90 || L % 18) L = 0;
    hop = L / 18;
    if (L == 0 || !(q >= q_min)) return PW_LOST;
    return L > n_sym - c ? PW_END : -1;
}

__device__ __forceinline__ void pw_res(int32_t *__restrict__ RES, int n, int next, int status) { RES[0] = n; RES[1] = next; RES[2] = status; RES[3] = 0; }

}  // namespace

__global__ void __launch_bounds__(256)
pls_walk_init_kernel(const int32_t *__restrict__ PLS, const float *__restrict__ MET, const float *__restrict__ ENE, const int32_t *__restrict__ LEN, int M, int start, int n_sym,
                     float q_min, int32_t *__restrict__ jump0, int32_t *__restrict__ rank)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    int32_t v, hop; float q;
    const int stop = pw_node(PLS, MET, ENE, LEN, i, start + 18 * i, n_sym, q_min, v, q, hop);
    jump0[i] = stop < 0 && hop < M - i ? i + hop : M;
    rank[i] = i == 0 ? 0 : -1;
}

__global__ void __launch_bounds__(256)
pls_walk_double_kernel(const int32_t *__restrict__ jk, int32_t *__restrict__ jn, int M)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int32_t j = jk[i];
    jn[i] = j < M ? jk[j] : M;
}

__global__ void __launch_bounds__(256)
pls_walk_mark_kernel(const int32_t *__restrict__ jk, int32_t *rank, int M, int step)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int32_t r = rank[i];
    if (r < 0) return;
    const int32_t j = jk[i];
    if (j < M) rank[j] = r + step;
}

__global__ void __launch_bounds__(256)
pls_walk_emit_kernel(const int32_t *__restrict__ PLS, const float *__restrict__ MET, const float *__restrict__ ENE, const int32_t *__restrict__ LEN, const int32_t *__restrict__ rank,
                     int M, int start, int n_sym, float q_min, int max_out, int32_t *__restrict__ OFF, int32_t *__restrict__ VAL, float *__restrict__ Q, int32_t *__restrict__ RES)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (M == 0) { if (i == 0) pw_res(RES, 0, start, PW_END); return; }      // not one whole header behind `start`
    if (i >= M) return;
    const int32_t r = rank[i];
    if (r < 0 || r > max_out) return;
    const int c = start + 18 * i;
    int32_t v, hop; float q;
    const int stop = pw_node(PLS, MET, ENE, LEN, i, c, n_sym, q_min, v, q, hop);
    if (stop >= 0) { pw_res(RES, r, c, stop); return; }
    if (r == max_out) { pw_res(RES, r, c, PW_FULL); return; }
    OFF[r] = c; VAL[r] = v; Q[r] = q;
    if (hop >= M - i) pw_res(RES, r + 1, c + 18 * hop, PW_END);              // the next header would begin past n_sym - 90 (c + 18 hop <= n_sym: this node is a frame)
}

// the same walk, lane 0 of one wave
__global__ void __launch_bounds__(64)
pls_walk_lane_kernel(const int32_t *__restrict__ PLS, const float *__restrict__ MET, const float *__restrict__ ENE, const int32_t *__restrict__ LEN, int M, int start, int n_sym,
                     float q_min, int max_out, int32_t *__restrict__ OFF, int32_t *__restrict__ VAL, float *__restrict__ Q, int32_t *__restrict__ RES)
{
    if (threadIdx.x != 0) return;
    int i = 0, j = 0, status = PW_END;
    while (i < M) {
        int32_t v, hop; float q;
        const int stop = pw_node(PLS, MET, ENE, LEN, i, start + 18 * i, n_sym, q_min, v, q, hop);
        if (stop >= 0) { status = stop; break; }
        if (j == max_out) { status = PW_FULL; break; }
        OFF[j] = start + 18 * i; VAL[j] = v; Q[j] = q;
        i += hop; j++;
    }
    pw_res(RES, j, start + 18 * i, status);
}

__global__ void __launch_bounds__(256)
pls_walk_group_kernel(const float2 *__restrict__ x, const int32_t *__restrict__ OFF, const int32_t *__restrict__ VAL, const int32_t *__restrict__ RES,
                      int32_t *__restrict__ CNT, int32_t *__restrict__ IDX, const float2 **__restrict__ SRC)
{
    __shared__ int32_t sv[PW_TILE], so[PW_TILE];
    __shared__ int32_t ss[256];
    const int t = threadIdx.x, N = RES[0];
    int cnt = 0;
    for (int j0 = 0; j0 < N; j0 += PW_TILE) {
        const int n = min(PW_TILE, N - j0);
        for (int k = t; k < n; k += 256) sv[k] = VAL[j0 + k];
        __syncthreads();
        for (int k = 0; k < n; k++) cnt += sv[k] == t;
        __syncthreads();
    }
    CNT[t] = cnt;
    // the group's first entry: the counts of the smaller values
    ss[t] = cnt;
    __syncthreads();
    for (int d = 1; d < 256; d *= 2) {
        const int a = t >= d ? ss[t - d] : 0;
        __syncthreads();
        ss[t] += a;
        __syncthreads();
    }
    int g = ss[t] - cnt;
    for (int j0 = 0; j0 < N; j0 += PW_TILE) {
        const int n = min(PW_TILE, N - j0);
        for (int k = t; k < n; k += 256) { sv[k] = VAL[j0 + k]; so[k] = OFF[j0 + k]; }
        __syncthreads();
        for (int k = 0; k < n; k++)
            if (sv[k] == t) {
                IDX[g] = j0 + k;
                if (SRC) SRC[g] = x + so[k];
                g++;
            }
        __syncthreads();
    }
}

int pls_walk_levels(int M, int min_hop, int max_out)
{
    const long long frames = M > 0 ? (M - 1) / min_hop + 1 : 0;                 // the most frames M candidates hold: the last rank a node can have
    const long long top = std::min<long long>(frames, max_out);
    int K = 0;
    while ((1ll << K) <= top) K++;
    return K;
}

size_t pls_walk_work_bytes(int M, int K) { return sizeof(int32_t) * (size_t)M * (size_t)(4 + std::max(K, 1)); }

// work: pls_walk_work_bytes(M, K) bytes -- PLS, MET, ENE of the M candidates (filled by the caller), the ranks, K levels of jumps.  lane: the one-lane walk
hipError_t pls_walk_launch(const float *X, int n_sym, int start, int M, int K, bool lane, const int32_t *LEN, float q_min, int max_out, void *work, int32_t *OFF, int32_t *VAL,
                           float *Q, const float **SRC, int32_t *IDX, int32_t *CNT, int32_t *RES, hipStream_t s)
{
    int32_t *pls = (int32_t *)work, *rank = pls + 3 * (size_t)M, *jump = pls + 4 * (size_t)M;
    const float *met = (const float *)work + M, *ene = (const float *)work + 2 * (size_t)M;
    const dim3 grid((unsigned)std::max((M + 255) / 256, 1)), blk(256);
    hipError_t e;
    if (lane) {
        hipLaunchKernelGGL(pls_walk_lane_kernel, dim3(1), dim3(64), 0, s, pls, met, ene, LEN, M, start, n_sym, q_min, max_out, OFF, VAL, Q, RES);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    } else {
        if (M > 0) {
            hipLaunchKernelGGL(pls_walk_init_kernel, grid, blk, 0, s, pls, met, ene, LEN, M, start, n_sym, q_min, jump, rank);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            for (int k = 0; k + 1 < K; k++) {
                hipLaunchKernelGGL(pls_walk_double_kernel, grid, blk, 0, s, jump + (size_t)k * M, jump + (size_t)(k + 1) * M, M);
                if ((e = hipGetLastError()) != hipSuccess) return e;
            }
            for (int k = K - 1; k >= 0; k--) {
                hipLaunchKernelGGL(pls_walk_mark_kernel, grid, blk, 0, s, jump + (size_t)k * M, rank, M, 1 << k);
                if ((e = hipGetLastError()) != hipSuccess) return e;
            }
        }
        hipLaunchKernelGGL(pls_walk_emit_kernel, grid, blk, 0, s, pls, met, ene, LEN, rank, M, start, n_sym, q_min, max_out, OFF, VAL, Q, RES);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(pls_walk_group_kernel, dim3(1), blk, 0, s, reinterpret_cast<const float2 *>(X), OFF, VAL, RES, CNT, IDX, reinterpret_cast<const float2 **>(SRC));
    return hipGetLastError();
}

}  // namespace dvbs2
