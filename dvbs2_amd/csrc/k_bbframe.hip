// BBFRAME layer (EN 302 307-1 clause 5.1, mode adaptation): user packets -> BBHEADER | DATA FIELD | padding on the way out, and back to packets on the way in.  An
// extension: the reference ends in K_bch anonymous bits per frame and has no such task.  The formats and the receiver's sequential rule are in include/dvbs2hip.h; this
// file is how the GPU reproduces them byte for byte.
//
// A frame's bits are one int32 each (the sockets of the chain), bit 8k of a frame the most significant bit of its byte k.  A lane turns 8 of them into a byte with two
// 16-byte loads (bits_byte); 64 lanes read 64 consecutive bytes of a frame, 2 KB of the socket.
//
// CRC-8, g(x) = x^8 + x^7 + x^6 + x^4 + x^2 + 1, register 0 at the start, nothing reflected: the CRC of the bytes b[0 .. n) is sum_t b[t] X^(n - t) mod g with X = x^8.
// It is linear, so a wave splits it over its lanes: lane l takes the bytes t = l, l + 64, ... in Horner form (times X^64 from one to the next), multiplies by its own
// X^(n - t_last), and six xor steps across the wave add the lanes up (wave_crc8).  A CRC that goes on from a register value r over n more bytes adds r X^n.  Products
// mod g are eight shift / xor steps (gf_mul): no table, neither in LDS nor per thread.
//
// Transmitter, bbf_build_kernel: one workgroup per frame.  The stream position of every byte of the call follows from the carried `pos`, so a frame knows its SYNCD
// and which of its bytes are CRC slots without looking at another frame; the CRC that goes into a slot covers the UPLB - 1 bytes in front of it, which the wave reads
// from the stream in global memory wherever the frame border falls.  Only the call's first slot (its packet began in an earlier call) needs the carried register.  The
// frame's bytes are put together in LDS and leave as bits, 16 bytes per lane and store.  The last workgroup writes the state behind the call.
//
// Receiver, three launches whatever F:
//   bbf_header_kernel  a wave per frame: the ten header bytes, their CRC-8, the fields, the frame's status
//   bbf_plan_kernel    one workgroup: the rule of include/dvbs2hip.h looks back one frame only -- a frame that is dropped or carries SYNCD = 65535 leaves no pending
//                      packet, every other frame leaves L - s - floor((L - s - 1) / UPLB) UPLB bytes -- so what frame f emits follows from the headers of f - 1 and f
//                      (the carried state for f = 0); a scan over the F counts gives every frame its place in the output, and the counters, N_OUT and the new
//                      `have` / length come out of the same pass (every packet counted as right: bbf_emit_kernel moves the wrong ones over)
//   bbf_emit_kernel    a workgroup per frame, a wave per packet: bytes from the bits (the head of a completed packet from the previous frame's tail, or from the
//                      carried bytes in frame 0), the CRC-8 over bytes 1 .. UPLB - 1 against the slot's byte, the packet and its status out; the last frame's
//                      workgroup saves the pending bytes
// State is read from one buffer and written to the other (the handle's ping-pong), so no workgroup reads what another one of the same launch writes.
#include "dvbs2hip_internal.h"
#include "rx_device.h"      // wave_xor

namespace dvbs2 {

namespace {

constexpr uint32_t CRC8_G = 0x1D5, CRC8_X = 0xD5;      // g(x), and X = x^8 mod g

// a b mod g for a, b of degree < 8
__host__ __device__ constexpr uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 7; i >= 0; i--) {
        r = (r << 1) ^ ((r & 0x80) ? CRC8_G : 0u);
        r ^= ((b >> i) & 1) ? a : 0u;
    }
    return r;
}
// X^m mod g
__host__ __device__ constexpr uint32_t gf_pow8(uint32_t m)
{
    uint32_t r = 1, b = CRC8_X;
    for (; m; m >>= 1) {
        if (m & 1) r = gf_mul(r, b);
        b = gf_mul(b, b);
    }
    return r;
}
constexpr uint32_t CRC8_X64 = gf_pow8(64);
static_assert(gf_mul(gf_mul(gf_mul(0x31, CRC8_X) ^ 0x32, CRC8_X) ^ 0x33, CRC8_X) == gf_mul(0x31, gf_pow8(3)) ^ gf_mul(0x32, gf_pow8(2)) ^ gf_mul(0x33, CRC8_X), "CRC-8: byte-wise = weighted sum");

// the CRC register after one more byte
__device__ __forceinline__ uint32_t crc8_step(uint32_t r, uint32_t b) { return gf_mul(r ^ b, CRC8_X); }

// lane l's factor for a CRC over n bytes: X^(n - t_last), t_last the last of l, l + 64, ... below n (no byte: 0)
__device__ __forceinline__ uint32_t crc8_lane_fac(int n, int lane)
{
    if (lane >= n) return 0;
    return gf_pow8((uint32_t)(n - (lane + (n - 1 - lane) / 64 * 64)));
}
__device__ __forceinline__ uint32_t wave_xor_all(uint32_t v)
{
    v ^= wave_xor<1>(v); v ^= wave_xor<2>(v); v ^= wave_xor<4>(v); v ^= wave_xor<8>(v); v ^= wave_xor<16>(v); v ^= wave_xor<32>(v);
    return v;
}
// CRC-8 over src[t], t in [0, n), bytes below t_lo taken as zero and not read (leading zeros leave the CRC alone); the whole wave calls it, every lane gets the result
__device__ __forceinline__ uint32_t wave_crc8(const uint8_t *src, int t_lo, int n, uint32_t fac, int lane)
{
    uint32_t acc = 0;
    for (int t = lane; t < n; t += 64) acc = gf_mul(acc, CRC8_X64) ^ (t >= t_lo ? (uint32_t)src[t] : 0u);
    return wave_xor_all(gf_mul(acc, fac));
}

typedef int32_t bbf_i4 __attribute__((ext_vector_type(4)));

// eight bits of a frame, first bit the most significant; `bits` is 32-byte aligned (a byte border of a frame whose socket is 16-byte aligned: K_bch is a multiple of 8)
__device__ __forceinline__ uint32_t bits_byte(const int32_t *bits)
{
    const bbf_i4 a = *reinterpret_cast<const bbf_i4 *>(bits), b = *reinterpret_cast<const bbf_i4 *>(bits + 4);
    return (a.x ? 128u : 0u) | (a.y ? 64u : 0u) | (a.z ? 32u : 0u) | (a.w ? 16u : 0u) | (b.x ? 8u : 0u) | (b.y ? 4u : 0u) | (b.z ? 2u : 0u) | (b.w ? 1u : 0u);
}

// ------------------------------------------------------------------ transmitter
// what goes into the CRC slot at stream byte j of the call (a packet starts there): the CRC-8 of the UPLB - 1 bytes in front of it
__device__ __forceinline__ uint32_t bbf_slot_value(const uint8_t *UP, long long j, int uplb, uint32_t fac_full, uint32_t run0, uint32_t last0, int lane)
{
    if (j == 0) return last0;                                                                        // the packet before it ended with the previous call
    if (j >= uplb - 1) return wave_crc8(UP + (j - uplb), 1, uplb, fac_full, lane);                   // all its bytes 1 .. UPLB - 1 are in this call
    return wave_crc8(UP, 0, (int)j, crc8_lane_fac((int)j, lane), lane) ^ gf_mul(run0, gf_pow8((uint32_t)j));      // it began in an earlier call: go on from the carried register
}

}  // namespace

__global__ void __launch_bounds__(256) bbf_build_kernel(const uint8_t *__restrict__ UP, long long n_bytes, int32_t *__restrict__ U, const int32_t *__restrict__ st_in,
                                                        int32_t *__restrict__ st_out, BbfParams p, int F)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t bbf_fr[];      // the frame's K / 8 bytes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.x;
    const int K = p.K, uplb = p.uplb, D = (K - 80) / 8;
    const long long j0 = (long long)f * D;
    const int len = (int)(n_bytes - j0 < D ? n_bytes - j0 : D);                                       // data bytes of this frame (the host checked 1 <= len)
    const int pos0 = st_in[0];
    const uint32_t run0 = (uint32_t)st_in[1], last0 = (uint32_t)st_in[2];
    const int pf = (int)((pos0 + j0) % uplb), d = (uplb - pf) % uplb;                                 // the first packet start of this frame is its byte d
    const uint32_t fac_full = crc8_lane_fac(uplb, lane);

    if (tid == 0) {
        const int dfl = 8 * len, syncd = 8 * d < dfl ? 8 * d : 65535, upl = 8 * uplb;
        const uint32_t hb[9] = {(uint32_t)p.matype >> 8 & 255u, (uint32_t)p.matype & 255u, (uint32_t)upl >> 8, (uint32_t)upl & 255u, (uint32_t)dfl >> 8, (uint32_t)dfl & 255u,
                                (uint32_t)p.sync, (uint32_t)syncd >> 8, (uint32_t)syncd & 255u};
        uint32_t r = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) { bbf_fr[k] = (uint8_t)hb[k]; r = crc8_step(r, hb[k]); }
        bbf_fr[9] = (uint8_t)r;
    }
    for (int t = tid; t < D; t += 256) bbf_fr[10 + t] = t < len ? UP[j0 + t] : (uint8_t)0;
    __syncthreads();
    for (int t = d + wave * uplb; t < len; t += 4 * uplb) {
        const uint32_t v = bbf_slot_value(UP, j0 + t, uplb, fac_full, run0, last0, lane);
        if (lane == 0) bbf_fr[10 + t] = (uint8_t)v;
    }
    __syncthreads();
    bbf_i4 *out = reinterpret_cast<bbf_i4 *>(U + (size_t)f * K);
    for (int w = tid; w < K / 4; w += 256) {
        const uint32_t by = bbf_fr[w >> 1], nib = (w & 1) ? by & 15u : by >> 4;
        bbf_i4 v;
        v.x = (int32_t)(nib >> 3 & 1u); v.y = (int32_t)(nib >> 2 & 1u); v.z = (int32_t)(nib >> 1 & 1u); v.w = (int32_t)(nib & 1u);
        out[w] = v;
    }
    if (f == F - 1 && wave == 0) {                                                                    // the state behind the call's last byte
        const int pos1 = (int)((pos0 + n_bytes) % uplb);
        uint32_t run1 = 0, last1 = last0;
        if (pos1 > 1) {
            if (n_bytes >= pos1 - 1) run1 = wave_crc8(UP + (n_bytes - pos1), 1, pos1, crc8_lane_fac(pos1, lane), lane);
            else run1 = wave_crc8(UP, 0, (int)n_bytes, crc8_lane_fac((int)n_bytes, lane), lane) ^ gf_mul(run0, gf_pow8((uint32_t)n_bytes));
        }
        if (n_bytes - pos1 > 0) last1 = bbf_slot_value(UP, n_bytes - pos1, uplb, fac_full, run0, last0, lane);      // the last packet that ended in this call
        if (lane == 0) { st_out[0] = pos1; st_out[1] = (int32_t)run1; st_out[2] = (int32_t)last1; st_out[3] = 0; }
    }
}

// ------------------------------------------------------------------ receiver
// the header record of a frame, eight int32: {status, MATYPE, UPL, DFL, SYNC, SYNCD, CRC-8 received, CRC-8 computed}
__global__ void __launch_bounds__(256) bbf_header_kernel(const int32_t *__restrict__ V, const int8_t *__restrict__ VALID, int32_t *__restrict__ hdr, int32_t *__restrict__ HDR,
                                                         BbfParams p, int F)
{
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= F) return;
    const uint32_t b = lane < 10 ? bits_byte(V + (size_t)f * p.K + 8 * lane) : 0u;
    uint32_t hb[10];
#pragma unroll
    for (int k = 0; k < 10; k++) hb[k] = (uint32_t)__builtin_amdgcn_readlane((int)b, k);
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) r = crc8_step(r, hb[k]);
    const int matype = (int)(hb[0] << 8 | hb[1]), upl = (int)(hb[2] << 8 | hb[3]), dfl = (int)(hb[4] << 8 | hb[5]), sync = (int)hb[6], syncd = (int)(hb[7] << 8 | hb[8]);
    int status = 0;
    if (VALID && VALID[f] == 0) status = 3;
    else if (r != hb[9]) status = 1;
    else if (upl != 8 * p.uplb || sync != p.sync || dfl > p.K - 80 || (dfl & 7) || (syncd != 65535 && ((syncd & 7) || syncd >= dfl))) status = 2;
    if (lane < 8) {
        const int v = lane == 0 ? status : lane == 1 ? matype : lane == 2 ? upl : lane == 3 ? dfl : lane == 4 ? sync : lane == 5 ? syncd : lane == 6 ? (int)hb[9] : (int)r;
        hdr[(size_t)f * 8 + lane] = v;
        if (HDR) HDR[(size_t)f * 8 + lane] = v;
    }
}

// the pending packet a frame leaves: {1, its bytes} or {0, 0}
static __device__ __forceinline__ void bbf_tail(const int32_t *h, int uplb, int &have, int &len)
{
    have = 0; len = 0;
    if (h[0] != 0 || h[5] == 65535) return;
    const int L = h[3] >> 3, s = h[5] >> 3;
    have = 1; len = L - s - (L - s - 1) / uplb * uplb;
}

// plan[f] = {place of the frame's first packet in the output, 1 = the frame completes the pending packet, packets that lie inside it, bytes of the pending packet}
__global__ void __launch_bounds__(256) bbf_plan_kernel(const int32_t *__restrict__ hdr, const int32_t *__restrict__ st_in, int32_t *__restrict__ st_out, bbf_i4 *__restrict__ plan,
                                                       int32_t *__restrict__ N_OUT, unsigned long long *__restrict__ ctr, int uplb, int F)
{
    __shared__ int wsum[4];
    __shared__ unsigned long long acc[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 3) acc[tid] = 0;
    int base = 0;
    unsigned taken = 0, dropped = 0;
    unsigned long long disc = 0;
    for (int f0 = 0; f0 < F; f0 += 256) {
        const int f = f0 + tid;
        int c = 0, complete = 0, n_emit = 0, len_in = 0;
        if (f < F) {
            int have;
            if (f == 0) { have = st_in[0]; len_in = have ? st_in[1] : 0; }
            else bbf_tail(hdr + (size_t)(f - 1) * 8, uplb, have, len_in);
            const int32_t *h = hdr + (size_t)f * 8;
            if (h[0] != 0) { dropped++; disc += (unsigned)len_in; }
            else {
                taken++;
                const int L = h[3] >> 3;
                if (h[5] == 65535) disc += (unsigned)(len_in + L);
                else {
                    const int s = h[5] >> 3;
                    complete = have && len_in + s == uplb;
                    if (!complete) disc += (unsigned)(len_in + s);
                    n_emit = (L - s - 1) / uplb;
                    c = complete + n_emit;
                }
            }
            if (f == F - 1) { int h1, l1; bbf_tail(h, uplb, h1, l1); st_out[0] = h1; st_out[1] = l1; st_out[2] = 0; st_out[3] = 0; }
        }
        int v = c;                                                                                    // inclusive scan over the workgroup
#pragma unroll
        for (int dlt = 1; dlt < 64; dlt <<= 1) { const int t = __shfl_up(v, dlt); if (lane >= dlt) v += t; }
        __syncthreads();                                                                              // (the previous round's wsum has been read)
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) { before += w < wave ? wsum[w] : 0; total += wsum[w]; }
        if (f < F) { bbf_i4 pl; pl.x = base + before + v - c; pl.y = complete; pl.z = n_emit; pl.w = len_in; plan[f] = pl; }
        base += total;
    }
    if (taken) atomicAdd(&acc[0], (unsigned long long)taken);
    if (dropped) atomicAdd(&acc[1], (unsigned long long)dropped);
    if (disc) atomicAdd(&acc[2], disc);
    __syncthreads();
    // every packet is counted as right here; bbf_emit_kernel moves the wrong ones over, which are few: one atomic per packet on one address costs more than the copy
    if (tid == 0) { ctr[0] += acc[0]; ctr[1] += acc[1]; ctr[2] += (unsigned long long)base; ctr[4] += acc[2]; *N_OUT = base; }
}

__global__ void __launch_bounds__(256) bbf_emit_kernel(const int32_t *__restrict__ V, const int32_t *__restrict__ hdr, const bbf_i4 *__restrict__ plan,
                                                       const uint8_t *__restrict__ st_in, uint8_t *__restrict__ st_out, uint8_t *__restrict__ UP, uint8_t *__restrict__ STATUS,
                                                       unsigned long long *__restrict__ ctr, BbfParams p, int cap, int F)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.x;
    const int K = p.K, uplb = p.uplb;
    const bbf_i4 pl = plan[f];
    const int off = pl.x, complete = pl.y, n = pl.y + pl.z, len_in = pl.w;
    const int32_t *h = hdr + (size_t)f * 8;
    const int L = h[3] >> 3, s = h[5] >> 3;                                                          // (read only where the plan says the frame is taken)
    const int32_t *df = V + (size_t)f * K + 80;
    // the pending packet's bytes: the previous frame's last len_in data bytes, in frame 0 the carried ones
    const int32_t *dfp = f > 0 ? V + (size_t)(f - 1) * K + 80 + 8 * (size_t)((hdr[(size_t)(f - 1) * 8 + 3] >> 3) - len_in) : nullptr;
    const uint8_t *carried = st_in + BBF_RX_HEAD;
    const uint32_t fac = crc8_lane_fac(uplb, lane);
    unsigned n_bad = 0;
    for (int k = wave; k < n; k += 4) {
        const int idx = off + k;
        if (idx >= cap) break;                                                                        // (cannot happen: dvbs2hip_bbframe_max_packets bounds the output; no store past it)
        const int start = (complete && k == 0) ? -len_in : s + (k - complete) * uplb;                 // packet byte q is data byte start + q
        uint8_t *out = UP + (size_t)idx * uplb;
        uint32_t acc = 0, first = 0, slot = 0;
        for (int q = lane; q <= uplb; q += 64) {
            const int t = start + q;
            const uint32_t b = t >= 0 ? bits_byte(df + 8 * (size_t)t) : f > 0 ? bits_byte(dfp + 8 * (size_t)q) : (uint32_t)carried[q];
            if (q < uplb) {
                out[q] = (uint8_t)(q == 0 ? (uint32_t)p.sync : b);
                acc = gf_mul(acc, CRC8_X64) ^ (q == 0 ? 0u : b);
                if (q == 1) first = b;
            } else slot = b;
        }
        const uint32_t crc = wave_xor_all(gf_mul(acc, fac));
        const uint32_t bad = crc != (uint32_t)__shfl((int)slot, uplb & 63);
        if (lane == 0) STATUS[idx] = (uint8_t)bad;
        if (bad && p.mark_tei && uplb == 188 && lane == 1) out[1] = (uint8_t)(first | 0x80u);       // transport_error_indicator
        n_bad += bad;
    }
    if (lane == 0 && n_bad) {                                                                         // (bbf_plan_kernel has counted them as right)
        atomicAdd(&ctr[3], (unsigned long long)n_bad);
        atomicAdd(&ctr[2], 0ull - (unsigned long long)n_bad);
    }
    if (f == F - 1) {                                                                                 // what the call leaves pending (bbf_plan_kernel wrote `have` and the length)
        int have, len;
        bbf_tail(h, uplb, have, len);
        for (int q = tid; q < len; q += 256) st_out[BBF_RX_HEAD + q] = (uint8_t)bits_byte(df + 8 * (size_t)(L - len + q));
    }
}

hipError_t bbframe_build_launch(const uint8_t *UP, long long n_bytes, int32_t *U, const int32_t *st_in, int32_t *st_out, const BbfParams &p, int F, hipStream_t s)
{
    const size_t lds = ((size_t)p.K / 8 + 15) / 16 * 16;
    hipLaunchKernelGGL(bbf_build_kernel, dim3(F), dim3(256), lds, s, UP, n_bytes, U, st_in, st_out, p, F);
    return hipGetLastError();
}

hipError_t bbframe_parse_launch(const int32_t *V, const int8_t *VALID, int32_t *hdr, int32_t *HDR, int32_t *plan, const uint8_t *st_in, uint8_t *st_out, uint8_t *UP,
                                uint8_t *STATUS, int32_t *N_OUT, unsigned long long *ctr, const BbfParams &p, int cap, int F, hipStream_t s)
{
    hipLaunchKernelGGL(bbf_header_kernel, dim3((F + 3) / 4), dim3(256), 0, s, V, VALID, hdr, HDR, p, F);
    hipLaunchKernelGGL(bbf_plan_kernel, dim3(1), dim3(256), 0, s, (const int32_t *)hdr, (const int32_t *)st_in, (int32_t *)st_out, (bbf_i4 *)plan, N_OUT, ctr, p.uplb, F);
    hipLaunchKernelGGL(bbf_emit_kernel, dim3(F), dim3(256), 0, s, V, (const int32_t *)hdr, (const bbf_i4 *)plan, st_in, st_out, UP, STATUS, ctr, p, cap, F);
    return hipGetLastError();
}

}  // namespace dvbs2
