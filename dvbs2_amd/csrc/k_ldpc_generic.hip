// a1 -- DVB-S2 LDPC decoder: the GENERIC table-driven kernel (per-slot flags, hybrid LDS/global image).  ONE FRAME = ONE WORKGROUP of 6 wavefronts,
// lane t = check t of the layer; the schedule, the compressed check->variable state and the storage policy are described in k_ldpc.hip, whose plan builds this
// kernel's tables (LdpcPlan::entries, groups, layer_lvl).  It is the fallback for codes the fast kernels reject -- check degree above 27 or more than 16
// duplicate edges per layer -- and the subject of `DVBS2HIP_LDPC_PATH=generic` experiments; every DVB-S2 code shipped here runs on k_ldpc_wg8.hip or
// k_ldpc_cu1.hip.  ldpc_dispatch.hip chooses between the three.  Behind it: the two small kernels of the work queue's opt-in frame order.
#include "ldpc_dispatch.h"
#include "ldpc_device.h"           // lds_float, const_u32 / const_i32 / const_u64 (and why they exist)

namespace dvbs2 {

// ------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------
static_assert(sizeof(LdpcGroup) == 8, "group table is read as 64-bit scalars");

__device__ __forceinline__ LdpcGroup group_ld(const_u64 groups, int g)
{
    const unsigned long long raw = groups[g];
    LdpcGroup v;
    v.base = (uint32_t)raw; v.lds = (uint32_t)(raw >> 32);
    return v;
}

// element (t - t0) mod 360 of the entry's bit-group, as a word offset into its store
__device__ __forceinline__ int ent_off(LdpcEntry e, int t)
{
    const int m = t - (int)(e & LE_T0_MASK);
    return (int)(((e >> LE_SLOT_SHIFT) & LE_SLOT_MASK) * LDPC_Z) + (int)min((unsigned)m, (unsigned)(m + LDPC_Z));
}
template <bool HYBRID>
__device__ __forceinline__ float post_ld(LdpcEntry e, int off, const lds_float *lpost, const float *gpost)
{
    if (HYBRID && !(e & LE_LDS)) return gpost[off];
    return lpost[off];
}
template <bool HYBRID>
__device__ __forceinline__ void post_st(LdpcEntry e, int off, lds_float *lpost, float *gpost, float v)
{
    if (HYBRID && !(e & LE_LDS)) gpost[off] = v;
    else lpost[off] = v;
}
// the edge does not exist for this lane (padding entry, or p_{c-1} of check 0)
__device__ __forceinline__ bool ent_absent(LdpcEntry e, int t) { return (e & LE_NULL) || ((e & LE_MASK0) && t == 0); }
__device__ __forceinline__ int ent_lvl(LdpcEntry e) { return (int)((e >> LE_LVL_SHIFT) & LE_LVL_MASK); }

// fp32 message from the packed per-check state: magnitude c1 at the slot of the minimum, c2
// elsewhere, sign bit j of pk
__device__ __forceinline__ float c2v_unpack(float c1, float c2, uint32_t pk, int j)
{
    const float mag = ((pk >> 27) == (uint32_t)j) ? c1 : c2;
    return __uint_as_float(__float_as_uint(mag) | ((pk << (31 - j)) & 0x80000000u));
}

template <int DEG, bool HYBRID, bool C2V_LDS>
__global__ void __launch_bounds__(LDPC_THREADS, (DEG > 13 && HYBRID) ? 2 : 3)      // (the 27-slot hybrid form needs ~172 registers: two waves per SIMD instead of three, no spills)
ldpc_layered_nms_kernel(const LdpcKParams p)
{
    extern __shared__ float smem[];
    lds_float *lpost = (lds_float *)smem;
    const int t = threadIdx.x;
    const bool act = t < LDPC_Z;
    const int M = p.M, q = p.q;
    const const_u32 entries = (const_u32)p.entries;
    const const_i32 layer_lvl = (const_i32)p.layer_lvl;
    const const_u64 groups = (const_u64)p.groups;

    for (int f = blockIdx.x; f < p.n_frames; f += gridDim.x) {
        const float *Y = p.llr + (size_t)f * p.N;
        float *gwork = p.gwork + (size_t)blockIdx.x * p.gwork_words;   // per-WORKGROUP slot: stays cache-hot across frames
        float *gpost = gwork;
        // packed c->v state [r][t]: two magnitudes + (5-bit min position | 27 sign bits).
        // Kept as two separately typed pointers (never a generic LDS-or-global pointer).
        lds_float *lc = lpost + p.lds_post_words;     // LDS image   (C2V_LDS)
        float *gc = gwork + p.glb_post_words;         // global image (!C2V_LDS)
#define C2V_LD(arr, i) (C2V_LDS ? lc[(arr) * M + (i)] : gc[(arr) * M + (i)])
#define C2V_ST(arr, i, val) do { if (C2V_LDS) lc[(arr) * M + (i)] = (val); else gc[(arr) * M + (i)] = (val); } while (0)

        // ---- load channel LLRs into the posterior stores (parity bits regrouped [r][t])
        if (act)
            for (int g = 0; g < p.n_groups; g++) {
                const LdpcGroup gl = group_ld(groups, g);
                const int src = g < p.n_info ? g * LDPC_Z + t : p.K + q * t + (g - p.n_info);
                const float v = Y[src];
                if (HYBRID && !gl.lds) gpost[gl.base + t] = v; else lpost[gl.base + t] = v;
            }
        for (int i = t; i < 3 * M; i += LDPC_THREADS) C2V_ST(0, i, 0.f);
        __syncthreads();

        int it = 0;
        bool ok = false;
        // the packed state of check (r, t) is private to lane t: prefetch the next layer's
        // while the current layer computes (global-memory latency off the critical path)
        float nx1 = 0.f, nx2 = 0.f, nxk = 0.f;
        if (act) { nx1 = C2V_LD(0, t); nx2 = C2V_LD(1, t); nxk = C2V_LD(2, t); }
        while (it < p.n_ite) {
            for (int r = 0; r < q; r++) {
                // the whole layer's table in SGPRs up front (unconditional, padded table)
                LdpcEntry E[DEG];
#pragma unroll
                for (int j = 0; j < DEG; j++) E[j] = entries[r * p.ent_stride + j];
                const int maxlvl = layer_lvl[r];
                const int ci = r * LDPC_Z + t;
                float v[DEG];
                float cst1 = 0.f, cst2 = 0.f, mn1 = INFINITY, mn2 = INFINITY;
                const float c1o = nx1, c2o = nx2;
                const uint32_t pko = __float_as_uint(nxk);
                uint32_t sacc = 0u;
                if (act) {
                    // ---- pass 1a: issue every posterior load of the check before using any
#pragma unroll
                    for (int j = 0; j < DEG; j++) v[j] = post_ld<HYBRID>(E[j], ent_off(E[j], t), lpost, gpost);
                    {
                        const int cn = (r + 1 < q ? ci + LDPC_Z : t);
                        nx1 = C2V_LD(0, cn); nx2 = C2V_LD(1, cn); nxk = C2V_LD(2, cn);
                    }
                    // ---- pass 1b: v->c = posterior - old c->v ; running min1/min2/sign
#pragma unroll
                    for (int j = 0; j < DEG; j++) {
                        float x = v[j] - c2v_unpack(c1o, c2o, pko, j);
                        if (ent_absent(E[j], t)) x = INFINITY;
                        v[j] = x;
                        const float a = fabsf(x);
                        mn2 = __builtin_amdgcn_fmed3f(mn1, mn2, a);
                        mn1 = fminf(mn1, a);
                        sacc ^= __float_as_uint(x);
                    }
                    cst1 = mn2 * p.alpha;
                    cst2 = mn1 * p.alpha;
                }
                if (maxlvl > 0) __syncthreads();      // every read of the layer precedes its writes
                uint32_t pkn = 0u, idxn = 0u;
                if (act) {
                    // ---- pass 2: new c->v ; posterior = v->c + new c->v (primary edges)
#pragma unroll
                    for (int j = 0; j < DEG; j++) {
                        const float x = v[j];
                        const bool ismin = fabsf(x) == mn1;
                        const float mag = ismin ? cst1 : cst2;
                        const uint32_t s = (sacc ^ __float_as_uint(x)) & 0x80000000u;
                        const float nw = __uint_as_float(__float_as_uint(mag) | s);
                        pkn |= s >> (31 - j);
                        idxn = ismin ? (uint32_t)j : idxn;
                        if (!ent_absent(E[j], t) && ent_lvl(E[j]) == 0)
                            post_st<HYBRID>(E[j], ent_off(E[j], t), lpost, gpost, x + nw);
                    }
                    pkn |= idxn << 27;
                    C2V_ST(0, ci, cst1); C2V_ST(1, ci, cst2); C2V_ST(2, ci, __uint_as_float(pkn));
                    if (q == 1) { nx1 = cst1; nx2 = cst2; nxk = __uint_as_float(pkn); }
                }
                // ---- duplicate edges of a bit-group inside this layer: ordered delta updates
                for (int lvl = 1; lvl <= maxlvl; lvl++) {
                    __syncthreads();
                    if (act) {
#pragma unroll
                        for (int j = 0; j < DEG; j++) {
                            if (ent_lvl(E[j]) == lvl && !(E[j] & LE_NULL)) {
                                const int off = ent_off(E[j], t);
                                const float nw = c2v_unpack(cst1, cst2, pkn, j);
                                const float od = c2v_unpack(c1o, c2o, pko, j);
                                const float L = post_ld<HYBRID>(E[j], off, lpost, gpost);
                                post_st<HYBRID>(E[j], off, lpost, gpost, L + (nw - od));
                            }
                        }
                    }
                }
                __syncthreads();
            }
            it++;
            if (p.early_stop || it == p.n_ite) {
                // ---- syndrome of the hard decisions (enable_syndrome, depth 1)
                int bad = 0;
                if (act)
                    for (int r = 0; r < q; r++) {
                        uint32_t x = 0u;
#pragma unroll
                        for (int j = 0; j < DEG; j++) {
                            const LdpcEntry e = entries[r * p.ent_stride + j];
                            const float L = post_ld<HYBRID>(e, ent_off(e, t), lpost, gpost);
                            x ^= (!ent_absent(e, t) && L < 0.f) ? 1u : 0u;
                        }
                        bad |= (int)x;
                    }
                ok = !__syncthreads_or(bad);
                if (ok) break;
            }
        }

        // ---- outputs
        if (t == 0) {
            if (p.cwd) p.cwd[f] = ok ? 1 : 0;
            if (p.ites) p.ites[f] = it;
        }
        if (act) {
            for (int g = 0; g < p.n_info; g++) {
                const LdpcGroup gl = group_ld(groups, g);
                const float L = (HYBRID && !gl.lds) ? gpost[gl.base + t] : lpost[gl.base + t];
                if (p.bits) p.bits[(size_t)f * p.K + g * LDPC_Z + t] = L < 0.f ? 1 : 0;
                if (p.post) p.post[(size_t)f * p.N + g * LDPC_Z + t] = L;
            }
            if (p.post)
                for (int g = p.n_info; g < p.n_groups; g++) {
                    const LdpcGroup gl = group_ld(groups, g);
                    const float L = (HYBRID && !gl.lds) ? gpost[gl.base + t] : lpost[gl.base + t];
                    p.post[(size_t)f * p.N + p.K + q * t + (g - p.n_info)] = L;
                }
        }
        if (p.packed) {
            // bit i of word w = info bit 32 w + i (tail bits zero); 360 = 11.25 words per group, so pack by word
            const int n_words = (p.K + 31) / 32;
            for (int w = t; w < n_words; w += LDPC_THREADS) {
                uint32_t word = 0u;
                for (int b = 0; b < 32; b++) {
                    const int k = 32 * w + b;
                    if (k >= p.K) break;
                    const int g = k / LDPC_Z, m = k - g * LDPC_Z;
                    const LdpcGroup gl = group_ld(groups, g);
                    const float L = (HYBRID && !gl.lds) ? gpost[gl.base + m] : lpost[gl.base + m];
                    word |= (L < 0.f ? 1u : 0u) << b;
                }
                p.packed[(size_t)f * n_words + w] = word;
            }
        }
        __syncthreads();     // LDS is reused by the next frame of this workgroup
    }
#undef C2V_LD
#undef C2V_ST
}

template <int DEG, bool HYBRID, bool C2V_LDS>
static hipError_t launch_inst(const LdpcPlan &pl, const LdpcKParams &p, hipStream_t s)
{
    const hipError_t e = ldpc_dyn_lds<ldpc_layered_nms_kernel<DEG, HYBRID, C2V_LDS>>(pl.lds_bytes);
    if (e != hipSuccess) return e;
    const int grid = p.n_frames < pl.grid_max ? p.n_frames : pl.grid_max;
    hipLaunchKernelGGL((ldpc_layered_nms_kernel<DEG, HYBRID, C2V_LDS>), dim3(grid), dim3(LDPC_THREADS), pl.lds_bytes, s, p);
    return hipGetLastError();
}

// resident workgroups per CU of an instantiation (persistent grid size)
template <int DEG, bool HYBRID, bool C2V_LDS>
static int occ_inst(const LdpcPlan &pl)
{
    auto kern = ldpc_layered_nms_kernel<DEG, HYBRID, C2V_LDS>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, LDPC_THREADS, pl.lds_bytes) != hipSuccess) nb = 1;
    return nb < 1 ? 1 : nb;
}
// every instantiation of the kernel, <DEG, HYBRID, C2V_LDS>
static_assert(LDPC_MAX_SLOTS == 27, "the table's second half is the LDPC_MAX_SLOTS form");
static const struct GenericInst { int targ[3]; hipError_t (*launch)(const LdpcPlan &, const LdpcKParams &, hipStream_t); int (*occ)(const LdpcPlan &); } generic_insts[] = {
    {{13, 0, 0}, launch_inst<13, false, false>, occ_inst<13, false, false>}, {{13, 0, 1}, launch_inst<13, false, true>, occ_inst<13, false, true>},
    {{13, 1, 0}, launch_inst<13, true, false>, occ_inst<13, true, false>},   {{13, 1, 1}, launch_inst<13, true, true>, occ_inst<13, true, true>},
    {{27, 0, 0}, launch_inst<27, false, false>, occ_inst<27, false, false>}, {{27, 0, 1}, launch_inst<27, false, true>, occ_inst<27, false, true>},
    {{27, 1, 0}, launch_inst<27, true, false>, occ_inst<27, true, false>},   {{27, 1, 1}, launch_inst<27, true, true>, occ_inst<27, true, true>},
};
static const GenericInst *generic_find(const int *targ)
{
    for (const GenericInst &i : generic_insts) if (i.targ[0] == targ[0] && i.targ[1] == targ[1] && i.targ[2] == targ[2]) return &i;
    return nullptr;
}
bool ldpc_generic_has(const int *targ) { return generic_find(targ) != nullptr; }
int ldpc_generic_blocks_per_cu(const LdpcPlan &pl, const LdpcChoice &ch) { const GenericInst *i = generic_find(ch.targ); return i ? i->occ(pl) : 1; }

hipError_t ldpc_generic_launch(const LdpcPlan &pl, const LdpcChoice &ch, LdpcKParams p, hipStream_t s)
{
    const GenericInst *i = generic_find(ch.targ);
    if (!i) return hipErrorInvalidValue;
    ldpc_plan_params(pl, p);
    p.entries = pl.d_entries; p.layer_deg = pl.d_layer_deg; p.layer_lvl = pl.d_layer_lvl; p.groups = pl.d_groups;
    p.ent_stride = pl.ent_stride; p.lds_post_words = pl.lds_post_words; p.glb_post_words = pl.glb_post_words;
    p.gwork_words = pl.gwork_words;
    return i->launch(pl, p, s);
}

// ------------------------------------------------------------------------------------------------------------------------------------------------------------
// (round 6; OPT-IN, DVBS2HIP_LDPC_ORDER=1: measured a 0.4 - 5 % LOSS, see dvbs2hip_api.hip ldpc_dev) Order in which the persistent grid's work queue hands out the frames
// of a launch with the stopping rule: noisiest first.  The idea: a frame that runs to the iteration cap takes 5 - 10 times the average, and one that starts last holds a
// workgroup while the chip idles; the mean |LLR| of a frame predicts those frames (tests/test_ldpc_gpu.py: 90 % of the noisier half do not converge).  The measurement:
// near the waterfall the AVERAGE frame already takes ~10 iterations and the counter-fed queue balances the rest -- there is no tail to hide.  Two small kernels in front of the
// decoder: sum |LLR| per frame (one streaming pass, ~0.1 ms per 8192 short frames), then a counting sort of the frames into 1024 buckets of that sum (one workgroup).
// Results do not depend on it: every frame is decoded exactly once, into its own sockets.
__global__ void __launch_bounds__(256)
frame_metric_kernel(const float *llr, float *metric, int N)
{
    const float *x = llr + (size_t)blockIdx.x * N;
    float a = 0.f;
    for (int i = threadIdx.x; i < N; i += 256) a += fabsf(x[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) metric[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ void __launch_bounds__(1024)
frame_order_kernel(const float *metric, uint32_t *order, int F)
{
    __shared__ uint32_t hist[1024], base[1024];
    __shared__ float red[2][16];
    const int t = threadIdx.x;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = t; i < F; i += 1024) { const float m = metric[i]; if (m == m && m < INFINITY) { lo = fminf(lo, m); hi = fmaxf(hi, m); } }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
    if ((t & 63) == 0) { red[0][t >> 6] = lo; red[1][t >> 6] = hi; }
    hist[t] = 0u;
    __syncthreads();
    lo = red[0][0]; hi = red[1][0];
    for (int k = 1; k < 16; k++) { lo = fminf(lo, red[0][k]); hi = fmaxf(hi, red[1][k]); }
    const float scale = hi > lo ? 1023.0f / (hi - lo) : 0.f;
    auto bucket = [&](float m) -> uint32_t { const float b = (m - lo) * scale; return b >= 0.f ? (b < 1023.f ? (uint32_t)b : 1023u) : 0u; };      // (NaN -> bucket 0: any bucket keeps `order` a permutation)
    for (int i = t; i < F; i += 1024) atomicAdd(&hist[bucket(metric[i])], 1u);
    __syncthreads();
    // exclusive prefix sum of the 1024 counts (Hillis-Steele in LDS)
    base[t] = hist[t];
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint32_t v = t >= o ? base[t - o] : 0u;
        __syncthreads();
        base[t] += v;
        __syncthreads();
    }
    const uint32_t excl = base[t] - hist[t];
    __syncthreads();
    base[t] = excl;
    __syncthreads();
    for (int i = t; i < F; i += 1024) order[atomicAdd(&base[bucket(metric[i])], 1u)] = (uint32_t)i;      // smallest sums (the noisiest frames) first
}

hipError_t frame_order_launch(const float *llr, float *metric, uint32_t *order, int F, int N, hipStream_t s)
{
    hipLaunchKernelGGL(frame_metric_kernel, dim3(F), dim3(256), 0, s, llr, metric, N);
    hipLaunchKernelGGL(frame_order_kernel, dim3(1), dim3(1024), 0, s, (const float *)metric, order, F);
    return hipGetLastError();
}

}  // namespace dvbs2
