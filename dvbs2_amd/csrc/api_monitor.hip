// C ABI, the monitor: error counters, their reduction across GPUs over RCCL (loaded at run time) and the file rendezvous of its bootstrap.
#include "dvbs2hip_handle.h"
#include <dlfcn.h>
#include <unistd.h>
#include <fcntl.h>
#include <time.h>
#include <chrono>
#include <thread>
#include <mutex>

using namespace dvbs2;

typedef struct { char internal[128]; } dvbs2hip_nccl_id;        // = ncclUniqueId (NCCL_UNIQUE_ID_BYTES = 128), passed by value

// ---- Monitor_reduction across GPUs (TX_RX_BB/main.cpp:123-125,155-161): one process per GPU, ONE RCCL all-reduce of 3 x uint64.
// librccl is opened at run time (the library itself does not link it: single-GPU users never load it).
namespace {
struct RcclApi {
    void *lib = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, dvbs2hip_nccl_id, int) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*CommAbort)(void *) = nullptr;      // optional
    const char *(*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;
std::mutex g_rccl_mutex;
const char *rccl_load()
{
    std::lock_guard<std::mutex> lock(g_rccl_mutex);      // two handles of one process may initialise their reductions from different threads
    if (g_rccl.lib) return nullptr;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void *l = nullptr;
    for (const char *n : names) if ((l = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;          // the copy the process already has (torch ships one)
    if (!l) for (const char *n : names) if ((l = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!l) return "librccl.so not found (dlopen)";
    g_rccl.GetUniqueId = (int (*)(void *))dlsym(l, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(void **, int, dvbs2hip_nccl_id, int))dlsym(l, "ncclCommInitRank");
    g_rccl.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(l, "ncclAllReduce");
    g_rccl.CommDestroy = (int (*)(void *))dlsym(l, "ncclCommDestroy");
    g_rccl.CommAbort = (int (*)(void *))dlsym(l, "ncclCommAbort");
    g_rccl.GetErrorString = (const char *(*)(int))dlsym(l, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy) return "librccl.so lacks the nccl* entry points";
    g_rccl.lib = l;
    return nullptr;
}
std::string rccl_err(int e) { return g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : ("rccl error " + std::to_string(e)); }
}  // namespace

// The out-of-band step of the RCCL bootstrap (no GPU involved; exported so that CPU processes can exercise it): rank 0 hands `bytes`
// bytes to every other rank through files named after `path`.  A file found under that name is never trusted for being there (a run
// that crashed leaves files behind, and a fixed name under /tmp can be squatted): every reader publishes a fresh random nonce in
// `path.hello.<rank>` and accepts only a `path.ack.<rank>` that carries the same nonce in front of the payload; rank 0 answers every
// hello it sees, answers again when a hello's nonce changes (a stale hello being replaced by the live reader's), and is done with a
// rank once that rank has consumed (removed) its ack.  Nothing is left behind by a successful exchange.  Files are created beside and
// renamed (nobody reads a partial file), with O_EXCL | O_NOFOLLOW and mode 0600; a private directory is still the better place.
namespace {
constexpr size_t RDV_NONCE = 16;
bool rdv_write(const std::string &name, const void *a, size_t na, const void *b, size_t nb)
{
    const std::string tmp = name + ".tmp." + std::to_string((long long)getpid());
    (void)unlink(tmp.c_str());
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW, 0600);
    if (fd < 0) return false;
    bool ok = (size_t)write(fd, a, na) == na && (nb == 0 || (size_t)write(fd, b, nb) == nb);
    ok = close(fd) == 0 && ok;
    if (ok) ok = rename(tmp.c_str(), name.c_str()) == 0;
    if (!ok) (void)unlink(tmp.c_str());
    return ok;
}
bool rdv_read(const std::string &name, void *buf, size_t n)      // true only for a regular file that holds exactly n bytes
{
    const int fd = open(name.c_str(), O_RDONLY | O_NOFOLLOW);
    if (fd < 0) return false;
    std::vector<unsigned char> tmp(n + 1);
    size_t got = 0;
    for (;;) { const ssize_t r = read(fd, tmp.data() + got, n + 1 - got); if (r <= 0) break; got += (size_t)r; if (got > n) break; }
    close(fd);
    if (got != n) return false;
    memcpy(buf, tmp.data(), n);
    return true;
}
void rdv_nonce(unsigned char *n)
{
    bool ok = false;
    const int fd = open("/dev/urandom", O_RDONLY);
    if (fd >= 0) { ok = read(fd, n, RDV_NONCE) == (ssize_t)RDV_NONCE; close(fd); }
    if (!ok) {
        struct timespec ts; clock_gettime(CLOCK_REALTIME, &ts);
        unsigned long long v[2] = {(unsigned long long)ts.tv_nsec ^ ((unsigned long long)getpid() << 32), (unsigned long long)ts.tv_sec ^ (unsigned long long)(uintptr_t)n};
        memcpy(n, v, RDV_NONCE);
    }
}
}  // namespace

extern "C" {

// ------------------------------------------------------------------ a9
int dvbs2hip_monitor_check_errors_dev(dvbs2hip_t *h, const int32_t *U, const int32_t *V, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!U || !V) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, monitor_launch(U, V, h->d_ctr, h->K_bch, F, h->stream));
    return 0;
}
int dvbs2hip_monitor_check_errors(dvbs2hip_t *h, const int32_t *U, const int32_t *V, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    const size_t n = (size_t)F * h->K_bch * 4;
    return host_call(h, F, false, {{U, B_IN, n}, {V, B_OUT, n}}, {},
                     [&](void *const *i, void *const *, int nf) { return dvbs2hip_monitor_check_errors_dev(h, (const int32_t *)i[0], (const int32_t *)i[1], nf); });
}
// check_errors2: the counters after every frame of the call, as sockets (device pointers; any of the five may be NULL)
int dvbs2hip_monitor_check_errors2_dev(dvbs2hip_t *h, const int32_t *U, const int32_t *V, int64_t *FRA, int32_t *BE, int32_t *FE, float *BER, float *FER, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    if (!U || !V) return fail(h, DVBS2HIP_EINVAL, "null socket pointer");
    void *tmp;
    if ((r = ensure(h, B_MON_BE, (size_t)F * 4, &tmp))) return r;
    Timer tm(h, DVBS2HIP_K_MISC);
    HIPCHK(h, monitor2_launch(U, V, h->d_ctr, (int32_t *)tmp, (long long *)FRA, BE, FE, BER, FER, h->K_bch, F, h->stream));
    return 0;
}
int dvbs2hip_monitor_check_errors2(dvbs2hip_t *h, const int32_t *U, const int32_t *V, int64_t *FRA, int32_t *BE, int32_t *FE, float *BER, float *FER, int32_t F)
{
    int r = check_frames(h, F); if (r) return r;
    const size_t n = (size_t)F * h->K_bch * 4, f4 = (size_t)F * 4;      // the five counters share one buffer: FRA (64-bit) first
    return host_call(h, F, false, {{U, B_IN, n}, {V, B_OUT, n}},
                     {{FRA, B_MON_OUT, 2 * f4, 0, true}, {BE, B_MON_OUT, f4, 2 * f4, true}, {FE, B_MON_OUT, f4, 3 * f4, true}, {BER, B_MON_OUT, f4, 4 * f4, true}, {FER, B_MON_OUT, f4, 5 * f4, true}},
                     [&](void *const *i, void *const *o, int nf) {
        return dvbs2hip_monitor_check_errors2_dev(h, (const int32_t *)i[0], (const int32_t *)i[1], (int64_t *)o[0], (int32_t *)o[1], (int32_t *)o[2], (float *)o[3], (float *)o[4], nf);
    });
}

int dvbs2hip_rendezvous(int32_t rank, int32_t world, const char *path, void *blob, size_t bytes, int32_t timeout_ms)
{
    if (world < 1 || rank < 0 || rank >= world || !path || !*path || !blob || !bytes) return DVBS2HIP_EINVAL;
    if (world == 1) return 0;
    const std::string base(path);
    const int step_ms = 20;
    if (rank > 0) {
        unsigned char nonce[RDV_NONCE];
        rdv_nonce(nonce);
        const std::string hello = base + ".hello." + std::to_string(rank), ack = base + ".ack." + std::to_string(rank);
        if (!rdv_write(hello, nonce, RDV_NONCE, nullptr, 0)) return fail(nullptr, DVBS2HIP_EINVAL, "cannot write the rendezvous file " + hello);
        std::vector<unsigned char> buf(RDV_NONCE + bytes);
        for (int waited = 0;; waited += step_ms) {
            if (rdv_read(ack, buf.data(), buf.size()) && !memcmp(buf.data(), nonce, RDV_NONCE)) {
                memcpy(blob, buf.data() + RDV_NONCE, bytes);
                (void)unlink(ack.c_str()); (void)unlink(hello.c_str());
                return 0;
            }
            if (timeout_ms >= 0 && waited >= timeout_ms) { (void)unlink(hello.c_str()); return fail(nullptr, DVBS2HIP_EHIP, "timed out waiting for rank 0 at the rendezvous " + base); }
            usleep(step_ms * 1000);
        }
    }
    std::vector<char> acked(world, 0), done(world, 0);
    std::vector<unsigned char> nonces((size_t)world * RDV_NONCE, 0);
    int left = world - 1;
    for (int waited = 0; left > 0; waited += step_ms) {
        for (int r = 1; r < world; r++) {
            if (done[r]) continue;
            const std::string hello = base + ".hello." + std::to_string(r), ack = base + ".ack." + std::to_string(r);
            unsigned char n[RDV_NONCE];
            if (rdv_read(hello, n, RDV_NONCE) && (!acked[r] || memcmp(n, &nonces[(size_t)r * RDV_NONCE], RDV_NONCE))) {
                if (!rdv_write(ack, n, RDV_NONCE, blob, bytes)) return fail(nullptr, DVBS2HIP_EINVAL, "cannot write the rendezvous file " + ack);
                memcpy(&nonces[(size_t)r * RDV_NONCE], n, RDV_NONCE); acked[r] = 1;
            } else if (acked[r] && access(ack.c_str(), F_OK) != 0) { done[r] = 1; left--; }      // consumed by its reader
        }
        if (left > 0) {
            if (timeout_ms >= 0 && waited >= timeout_ms) {
                for (int r = 1; r < world; r++) if (acked[r] && !done[r]) (void)unlink((base + ".ack." + std::to_string(r)).c_str());
                return fail(nullptr, DVBS2HIP_EHIP, "timed out waiting for " + std::to_string(left) + " rank(s) at the rendezvous " + base);
            }
            usleep(step_ms * 1000);
        }
    }
    return 0;
}

int dvbs2hip_monitor_reduce_init(dvbs2hip_t *h, int32_t rank, int32_t world, const char *rendezvous, int32_t timeout_ms)
{
    int r0 = enter(h); if (r0) return r0;
    if (world < 1 || rank < 0 || rank >= world) return fail(h, DVBS2HIP_EINVAL, "'rank' has to be in [0, world_size)");
    if (h->nccl_comm) return fail(h, DVBS2HIP_EINVAL, "the monitor reduction is already initialised on this handle");
    if (world > 1 && (!rendezvous || !*rendezvous)) return fail(h, DVBS2HIP_EINVAL, "a rendezvous file path is needed for world_size > 1");
    if (const char *e = rccl_load()) return fail(h, DVBS2HIP_EUNSUPPORTED, e);
    dvbs2hip_nccl_id id;
    memset(&id, 0, sizeof id);
    if (rank == 0) {
        int e = g_rccl.GetUniqueId(&id);
        if (e) return fail(h, DVBS2HIP_EHIP, "ncclGetUniqueId: " + rccl_err(e));
    }
    if (world > 1) {
        const int rr = dvbs2hip_rendezvous(rank, world, rendezvous, &id, sizeof id, timeout_ms);
        if (rr) return fail(h, rr, dvbs2hip_last_error(nullptr));
    }
    void *comm = nullptr;
    int e = g_rccl.CommInitRank(&comm, world, id, rank);
    if (e) return fail(h, DVBS2HIP_EHIP, "ncclCommInitRank: " + rccl_err(e));
    if (!h->d_red && dev_alloc(h, &h->d_red, 3 * sizeof(unsigned long long), "hipMalloc failed")) { (void)g_rccl.CommDestroy(comm); return DVBS2HIP_ENOMEM; }
    if (!h->h_red && hipHostMalloc((void **)&h->h_red, 3 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) { h->h_red = nullptr; (void)g_rccl.CommDestroy(comm); return fail(h, DVBS2HIP_ENOMEM, "hipHostMalloc failed"); }
    h->nccl_comm = comm; h->red_rank = rank; h->red_world = world; h->red_timeout_ms = timeout_ms > 0 ? timeout_ms : 0;
    return 0;
}

int dvbs2hip_monitor_reduce(dvbs2hip_t *h, uint64_t out[3])
{
    if (!h || !out) return DVBS2HIP_EINVAL;
    if (!h->nccl_comm) return dvbs2hip_monitor_get(h, out);         // a single process: the local counters are the sum
    int r0 = enter(h); if (r0) return r0;
    const int e = g_rccl.AllReduce(h->d_ctr, h->d_red, 3, 5 /* ncclUint64 */, 0 /* ncclSum */, h->nccl_comm, h->stream);
    if (e) return fail(h, DVBS2HIP_EHIP, "ncclAllReduce: " + rccl_err(e));
    unsigned long long *tmp = h->h_red;
    HIPCHK(h, hipMemcpyAsync(tmp, h->d_red, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    // A peer that died leaves this rank's all-reduce waiting on the device for ever: wait with the timeout given at _reduce_init instead of a blocking
    // synchronize -- a launcher-less `dvbs2_tx_rx_bb --world N` then ends with a non-zero exit code of its own instead of hanging until somebody kills it.
    if (h->red_timeout_ms > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t q = hipStreamQuery(h->stream);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) HIPCHK(h, q);
            if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > h->red_timeout_ms) {
                if (g_rccl.CommAbort) (void)g_rccl.CommAbort(h->nccl_comm);
                h->nccl_comm = nullptr; h->comm_dead = true;
                return fail(h, DVBS2HIP_ETIMEOUT, "monitor reduction: a peer rank did not arrive within " + std::to_string(h->red_timeout_ms) + " ms (rank " + std::to_string(h->red_rank) + " of " + std::to_string(h->red_world) + ")");
            }
            if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() >= 5) std::this_thread::sleep_for(std::chrono::microseconds(50));      // (spin for the first 5 ms: a reduction that arrives is microseconds away)
        }
    } else
        HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 3; i++) out[i] = tmp[i];
    return 0;
}

int dvbs2hip_monitor_reduce_finalize(dvbs2hip_t *h)
{
    if (!h) return DVBS2HIP_EINVAL;
    if (h->nccl_comm) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        (void)g_rccl.CommDestroy(h->nccl_comm);
        h->nccl_comm = nullptr; h->red_world = 1; h->red_rank = 0;
    }
    return 0;
}

int dvbs2hip_monitor_get(dvbs2hip_t *h, uint64_t out[3])
{
    if (!h || !out) return DVBS2HIP_EINVAL;
    int r0 = enter(h); if (r0) return r0;
    unsigned long long tmp[3];
    HIPCHK(h, hipMemcpyAsync(tmp, h->d_ctr, sizeof tmp, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 3; i++) out[i] = tmp[i];
    return 0;
}
int dvbs2hip_monitor_reset(dvbs2hip_t *h)
{
    int r0 = enter(h); if (r0) return r0;
    HIPCHK(h, hipMemsetAsync(h->d_ctr, 0, 3 * sizeof(unsigned long long), h->stream));
    return 0;
}

}  // extern "C"
