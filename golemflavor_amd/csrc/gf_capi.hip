// gf_capi.hip -- the entry points of the C ABI declared in include/golemflavor_hip.h: the library's error text and environment
// overrides, the host-buffer batches with their staging, the device-resident calls, haar draws, the histogram, copies and events.
// The model itself is gf_model.hip's, the per-device pools are gf_pool.hip's.  Host code only.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "gf_devcache.h"                // large device allocations are cached, not handed back to the driver
#include "gf_host.h"
#include "gf_model.h"

namespace {

thread_local char g_err[512] = "";      // reached through gf_internal_set_error / gf_last_hip_error only

// Every environment override the library honours goes through gf_internal_env and is REMEMBERED: gf_diagnostic_overrides()
// lists them, bench.py and scan.py print the list in their JSON line.  Overrides that can change a RESULT (the unitarity
// tiers' thresholds: a verdict; GF_UNI_DUMP: fr[0]) are honoured only when GF_DIAGNOSTICS=1 is set as well, so that a stray
// variable in somebody's shell cannot silently change what a run computes; ignoring one is reported once on stderr.
std::mutex g_env_mu;
char g_env_seen[1024] = "";

// device buffers for `n` rows, pinned mirror for `n_pin` rows (n_pin < n: the batch streams through the mirror in chunks)
int ensure_staging(gf_model* m, int64_t n, int64_t n_pin)
{
    const size_t nd = (size_t)m->c.ndim;
    if (n > m->cap) {
        int64_t cap = m->cap ? m->cap : 1024;
        while (cap < n) cap *= 2;
        if (m->d_theta) (void)gf_cached_free(m->d_theta);
        if (m->d_out) (void)gf_cached_free(m->d_out);
        if (m->d_status) (void)gf_cached_free(m->d_status);
        m->d_theta = nullptr; m->d_out = nullptr; m->d_status = nullptr; m->cap = 0;
        GF_HIP(gf_cached_malloc((void**)&m->d_theta, sizeof(double) * nd * cap));
        GF_HIP(gf_cached_malloc((void**)&m->d_out, sizeof(double) * 4 * cap));
        GF_HIP(gf_cached_malloc((void**)&m->d_status, sizeof(int32_t) * cap));
        m->cap = cap;
    }
    if (n_pin > m->hcap) {
        int64_t hcap = m->hcap ? m->hcap : 1024;
        while (hcap < n_pin) hcap *= 2;
        if (m->h_pin) (void)hipHostFree(m->h_pin);
        m->h_pin = nullptr; m->hcap = 0;
        m->h_pin_bytes = sizeof(double) * (nd + 4) * hcap + sizeof(int32_t) * hcap;
        GF_HIP(hipHostMalloc(&m->h_pin, m->h_pin_bytes, hipHostMallocDefault));
        m->hcap = hcap;
    }
    return GF_OK;
}

int check_dev_ptr(const void* p, size_t align)
{
    if (!p) return GF_ERR_INVALID_ARG;
    if (((uintptr_t)p) % align) return gf_fail_msg(GF_ERR_INVALID_ARG, "device pointer %p is not %zu-byte aligned", p, align);
    return GF_OK;
}

}  // namespace

extern "C" {

int gf_abi_version(void) { return GF_ABI_VERSION; }

const char* gf_strerror(int err)
{
    switch (err) {
    case GF_OK: return "ok";
    case GF_ERR_INVALID_ARG: return "invalid argument";
    case GF_ERR_NO_DEVICE: return "no gfx950 HIP device available (this library has no CPU fallback)";
    case GF_ERR_HIP: return "HIP runtime error";
    case GF_ERR_ALLOC: return "allocation failed";
    case GF_ERR_COMM: return "RCCL error";
    case GF_ERR_UNSUPPORTED: return "unsupported configuration";
    case GF_ERR_QUEUE_OVERFLOW: return "unitarity queue overflow";
    default: return "unknown error";
    }
}

const char* gf_last_hip_error(void) { return g_err; }

// internal (gf_sampler_host.hip, gf_comm.hip): one thread-local error text for the whole library
void gf_internal_set_error(const char* msg) { std::snprintf(g_err, sizeof(g_err), "%s", msg ? msg : ""); }

size_t gf_sizeof_model_desc(void) { return sizeof(gf_model_desc); }

// internal: getenv with a record.  `affects_results` != 0: honoured only under GF_DIAGNOSTICS=1.
const char* gf_internal_env(const char* name, int affects_results)
{
    const char* v = std::getenv(name);
    if (!v) return nullptr;
    std::lock_guard<std::mutex> lk(g_env_mu);
    char item[160];
    if (affects_results) {
        const char* d = std::getenv("GF_DIAGNOSTICS");
        if (!d || d[0] != '1') {
            std::snprintf(item, sizeof(item), "%s(ignored)", name);
            if (!std::strstr(g_env_seen, item)) {
                std::fprintf(stderr, "libgolemhip: %s is set but GF_DIAGNOSTICS=1 is not: ignored (it would change results)\n", name);
                if (std::strlen(g_env_seen) + std::strlen(item) + 2 < sizeof(g_env_seen)) { if (g_env_seen[0]) std::strcat(g_env_seen, " "); std::strcat(g_env_seen, item); }
            }
            return nullptr;
        }
    }
    std::snprintf(item, sizeof(item), "%s=%.100s", name, v);
    if (!std::strstr(g_env_seen, item) && std::strlen(g_env_seen) + std::strlen(item) + 2 < sizeof(g_env_seen)) {
        if (g_env_seen[0]) std::strcat(g_env_seen, " ");
        std::strcat(g_env_seen, item);
    }
    return v;
}

int gf_diagnostic_overrides(char* buf, size_t buflen)
{
    if (!buf || buflen == 0) return GF_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_env_mu);
    std::snprintf(buf, buflen, "%s", g_env_seen);
    return GF_OK;
}

int gf_device_count(int* count)
{
    if (!count) return GF_ERR_INVALID_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; (void)hipGetLastError(); return GF_OK; }
    *count = n;
    return GF_OK;
}

int gf_device_name(int device, char* buf, size_t buflen)
{
    if (!buf || buflen == 0) return GF_ERR_INVALID_ARG;
    hipDeviceProp_t prop;
    GF_HIP(hipGetDeviceProperties(&prop, device));
    std::snprintf(buf, buflen, "%s", prop.gcnArchName);
    return GF_OK;
}

// ---- host-buffer entry points ------------------------------------------------------------
// Rows per chunk of the large-batch pipeline, and the batch size from which it is used.  A large batch streams through two
// pinned slots: the host copies chunk c + 1 into its slot while chunk c crosses PCIe (and the other way round for the
// results).  Copying the whole batch into a pinned mirror first and transferring it then -- the path below this size, where
// it is one memcpy and one transfer -- runs at 1 / (1/33 + 1/57) = 21 GB/s on the MI355X box, the pipeline at the slower of
// the two (tools/h2d_probe.hip); the mirror of a 4 M-row batch also took 0.1 s to allocate (hipHostMalloc: 4.7 GB/s).
constexpr int64_t PIPE_CHUNK_ROWS = 65536;
constexpr int64_t PIPE_MIN_ROWS = 4 * PIPE_CHUNK_ROWS;
constexpr int64_t GF_ZEROCOPY_MAX_ROWS = 2048;

static void parallel_memcpy(char* dst, const char* src, size_t len) { gf_internal_copy_rows(dst, len, src, len, 1); }     // the host copy pool (gf_readback.hip)

// The results of a batch wherever they lie -- the caller's arrays (fr, and st, may be NULL: not asked for), the device staging, the
// pinned mirror: lnprob [n], composition [n][3], status [n]
struct Rows { double* ln; double* fr; int32_t* st; };
static Rows device_rows(const gf_model* m) { return {m->d_out, m->d_out + m->cap, m->d_status}; }
// the pinned mirror: theta [hcap][ndim] (or the smaller cube), then its three result regions
struct PinView { double* theta; Rows res; };
static PinView pin_view(const gf_model* m)
{
    double* h_theta = (double*)m->h_pin;
    double* h_out = h_theta + (size_t)m->c.ndim * m->hcap;
    double* h_fr = h_out + m->hcap;
    return {h_theta, {h_out, h_fr, (int32_t*)(h_fr + 3 * m->hcap)}};
}

// evaluate the n rows at `theta` on the model's stream into `to`: lnprob with what the caller asked for of fr / status, or the composition
static int evaluate(gf_model* m, bool with_llh, const double* theta, int64_t n, const Rows& to, const Rows& user)
{
    int32_t* st = user.st ? to.st : nullptr;
    return with_llh ? launch_lnprob(m, m->stream, theta, GF_LAYOUT_AOS, n, to.ln, user.fr ? to.fr : nullptr, st)
                    : launch_propagate(m, m->stream, theta, GF_LAYOUT_AOS, n, to.fr, st);
}

// the end of a batch of one piece: what the caller asked for comes down from `dev` into the pinned mirror (NULL: the kernel wrote
// the mirror itself), the stream is waited for, the mirror is copied out, and a queue overflow is reported
static int deliver(gf_model* m, bool with_llh, int64_t n, const Rows* dev, const Rows& pin, const Rows& user)
{
    if (dev) {
        if (with_llh) GF_HIP(hipMemcpyAsync(pin.ln, dev->ln, sizeof(double) * n, hipMemcpyDeviceToHost, m->stream));
        if (user.fr) GF_HIP(hipMemcpyAsync(pin.fr, dev->fr, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, m->stream));
        if (user.st) GF_HIP(hipMemcpyAsync(pin.st, dev->st, sizeof(int32_t) * n, hipMemcpyDeviceToHost, m->stream));
    }
    GF_HIP(hipStreamSynchronize(m->stream));
    if (with_llh) std::memcpy(user.ln, pin.ln, sizeof(double) * n);
    if (user.fr) std::memcpy(user.fr, pin.fr, sizeof(double) * 3 * n);
    if (user.st) std::memcpy(user.st, pin.st, sizeof(int32_t) * n);
    return user.st ? check_queue_overflow(m->device, m->stream) : GF_OK;
}

static int run_host_pipelined(gf_model* m, const double* theta, int64_t n, double* lnprob, double* fr, int32_t* status, bool with_llh)
{
    // From 2 M rows on the chunks are four times as long and the copies into and out of the slots are shared out over the
    // host copy pool (copy_rows: 1 MB pieces): one thread copies at 33 GB/s, PCIe takes 57 (round 3).
    const int64_t CH = n >= 32 * PIPE_CHUNK_ROWS ? 4 * PIPE_CHUNK_ROWS : PIPE_CHUNK_ROWS;
    int rc = ensure_staging(m, n, 2 * CH);
    if (rc != GF_OK) return rc;
    for (int k = 0; k < 2; ++k) {
        if (!m->ev_up[k]) GF_HIP(hipEventCreateWithFlags(&m->ev_up[k], hipEventDisableTiming));
        if (!m->ev_down[k]) GF_HIP(hipEventCreateWithFlags(&m->ev_down[k], hipEventDisableTiming));
    }
    const size_t nd = (size_t)m->c.ndim;
    const PinView pin = pin_view(m);
    double* const h_theta = pin.theta;
    double* const h_out = pin.res.ln;
    double* const h_fr = pin.res.fr;
    int32_t* const h_st = pin.res.st;
    const int64_t nchunks = (n + CH - 1) / CH;
    for (int64_t c = 0; c < nchunks; ++c) {
        const int slot = (int)(c & 1);
        const int64_t off = c * CH, len = n - off < CH ? n - off : CH;
        if (c >= 2) GF_HIP(hipEventSynchronize(m->ev_up[slot]));        // the slot's previous chunk has left for the device
        parallel_memcpy(reinterpret_cast<char*>(h_theta + nd * CH * slot), reinterpret_cast<const char*>(theta + nd * off), sizeof(double) * nd * len);
        GF_HIP(hipMemcpyAsync(m->d_theta + nd * off, h_theta + nd * CH * slot, sizeof(double) * nd * len, hipMemcpyHostToDevice, m->stream));
        GF_HIP(hipEventRecord(m->ev_up[slot], m->stream));
    }
    const Rows dev = device_rows(m);
    double* const d_ln = dev.ln;
    double* const d_fr = dev.fr;
    rc = evaluate(m, with_llh, m->d_theta, n, dev, {lnprob, fr, status});
    if (rc != GF_OK) return rc;
    // results: chunk c comes down into its slot while the host copies chunk c - 1 out of the other (the transfers follow the
    // kernel, and with it every upload that read these slots, in stream order)
    auto copy_out = [&](int64_t c) {
        const int slot = (int)(c & 1);
        const int64_t off = c * CH, len = n - off < CH ? n - off : CH;
        if (with_llh) parallel_memcpy(reinterpret_cast<char*>(lnprob + off), reinterpret_cast<const char*>(h_out + CH * slot), sizeof(double) * len);
        if (fr) parallel_memcpy(reinterpret_cast<char*>(fr + 3 * off), reinterpret_cast<const char*>(h_fr + 3 * CH * slot), sizeof(double) * 3 * len);
        if (status) parallel_memcpy(reinterpret_cast<char*>(status + off), reinterpret_cast<const char*>(h_st + CH * slot), sizeof(int32_t) * len);
    };
    for (int64_t c = 0; c < nchunks; ++c) {
        const int slot = (int)(c & 1);
        const int64_t off = c * CH, len = n - off < CH ? n - off : CH;
        if (with_llh) GF_HIP(hipMemcpyAsync(h_out + CH * slot, d_ln + off, sizeof(double) * len, hipMemcpyDeviceToHost, m->stream));
        if (fr) GF_HIP(hipMemcpyAsync(h_fr + 3 * CH * slot, d_fr + 3 * off, sizeof(double) * 3 * len, hipMemcpyDeviceToHost, m->stream));
        if (status) GF_HIP(hipMemcpyAsync(h_st + CH * slot, m->d_status + off, sizeof(int32_t) * len, hipMemcpyDeviceToHost, m->stream));
        GF_HIP(hipEventRecord(m->ev_down[slot], m->stream));
        if (c >= 1) {
            GF_HIP(hipEventSynchronize(m->ev_down[slot ^ 1]));
            copy_out(c - 1);
        }
    }
    GF_HIP(hipEventSynchronize(m->ev_down[(nchunks - 1) & 1]));
    copy_out(nchunks - 1);
    return status ? check_queue_overflow(m->device, m->stream) : GF_OK;
}

static int run_host(gf_model* m, const double* theta, int64_t n, double* lnprob, double* fr, int32_t* status,
                    bool with_llh)
{
    if (!m || n < 0 || (n > 0 && (!theta || (with_llh && !lnprob) || (!with_llh && !fr)))) return GF_ERR_INVALID_ARG;
    if (n == 0) return GF_OK;
    // one caller at a time per model: the staging buffers (and the arbitration queue) are the model's
    std::lock_guard<std::mutex> lk(m->call_mu);
    GF_STREAM(m);
    static const bool pipe_off = gf_internal_env("GF_NO_HOST_PIPELINE", 0) != nullptr;  // diagnostics / A-B
    if (n >= PIPE_MIN_ROWS && !pipe_off) return run_host_pipelined(m, theta, n, lnprob, fr, status, with_llh);
    int rc = ensure_staging(m, n, n);
    if (rc != GF_OK) return rc;
    const size_t nd = (size_t)m->c.ndim;
    const PinView pin = pin_view(m);
    const Rows user = {lnprob, fr, status};
    std::memcpy(pin.theta, theta, sizeof(double) * nd * n);
    // Small batches (emcee's half-ensemble of a 100-walker chain is 50 rows): the kernel reads theta from and
    // writes its results to the pinned, device-mapped staging buffer directly -- one launch and one stream
    // sync instead of launch + two DMA transfers, each of which costs more than the kilobytes they move.
    static const bool zc_off = gf_internal_env("GF_NO_ZEROCOPY", 0) != nullptr;       // diagnostics / A-B
    if (n <= GF_ZEROCOPY_MAX_ROWS && !zc_off) {
        rc = evaluate(m, with_llh, pin.theta, n, pin.res, user);
        return rc != GF_OK ? rc : deliver(m, with_llh, n, nullptr, pin.res, user);
    }
    GF_HIP(hipMemcpyAsync(m->d_theta, pin.theta, sizeof(double) * nd * n, hipMemcpyHostToDevice, m->stream));
    const Rows dev = device_rows(m);
    rc = evaluate(m, with_llh, m->d_theta, n, dev, user);
    return rc != GF_OK ? rc : deliver(m, with_llh, n, &dev, pin.res, user);
}

int gf_lnprob_batch(gf_model* m, const double* theta, int64_t n, double* lnprob, double* fr, int32_t* status)
{
    return run_host(m, theta, n, lnprob, fr, status, true);
}

// MultiNest-style batch (golemflavor/mn.py:26-45 lnProb): cube [n][nscan] in the unit cube; column cols[k] of theta is
// lo + (hi - lo) * cube[.][k] with the model's own box for that column, every other column is base[col].  The map runs
// on the device; only the cube crosses PCIe.
int gf_lnprob_cube_batch(gf_model* m, const double* cube, int64_t n, int nscan, const int32_t* cols, const double* base,
                         double* lnprob, double* fr, int32_t* status)
{
    if (!m || n < 0 || nscan < 1 || nscan > m->c.ndim || !cols || !base || (n > 0 && (!cube || !lnprob))) return GF_ERR_INVALID_ARG;
    bool seen[GF_MAX_DIM] = {false};
    for (int k = 0; k < nscan; ++k) {
        if (cols[k] < 0 || cols[k] >= m->c.ndim || seen[cols[k]]) return GF_ERR_INVALID_ARG;
        seen[cols[k]] = true;
    }
    if (n == 0) return GF_OK;
    std::lock_guard<std::mutex> lk(m->call_mu);
    GF_STREAM(m);
    int rc = ensure_staging(m, n, n);
    if (rc != GF_OK) return rc;
    const PinView pin = pin_view(m);
    double* h_cube = pin.theta;                              // the theta slot of the pinned mirror holds the (smaller) cube
    // device side: the cube rows get their own buffer, grown on demand (d_theta receives the expanded rows)
    if ((int64_t)m->cube_cap < n * nscan) {
        if (m->d_cube) (void)gf_cached_free(m->d_cube);
        m->d_cube = nullptr; m->cube_cap = 0;
        GF_HIP(gf_cached_malloc((void**)&m->d_cube, sizeof(double) * (size_t)n * nscan));
        m->cube_cap = (size_t)n * nscan;
    }
    std::memcpy(h_cube, cube, sizeof(double) * (size_t)n * nscan);
    GF_HIP(hipMemcpyAsync(m->d_cube, h_cube, sizeof(double) * (size_t)n * nscan, hipMemcpyHostToDevice, m->stream));
    hipError_t e = gf_launch_cube_to_theta(m->c, nscan, cols, base, m->d_cube, n, m->d_theta, m->cus, m->stream);
    if (e != hipSuccess) return gf_hip_fail(e, "cube map launch");
    const Rows dev = device_rows(m), user = {lnprob, fr, status};
    rc = evaluate(m, true, m->d_theta, n, dev, user);
    return rc != GF_OK ? rc : deliver(m, true, n, &dev, pin.res, user);
}

int gf_propagate_batch(gf_model* m, const double* theta, int64_t n, double* fr, int32_t* status)
{
    return run_host(m, theta, n, nullptr, fr, status, false);
}

int gf_haar_draw(gf_model* m, uint64_t seed, int64_t first_draw, int64_t n, double* angles, double* fr)
{
    if (!m || n < 0 || (n > 0 && !fr)) return GF_ERR_INVALID_ARG;
    if (n == 0) return GF_OK;
    GF_STREAM(m);
    double *d_fr = nullptr, *d_ang = nullptr;
    GF_HIP(gf_cached_malloc((void**)&d_fr, sizeof(double) * 3 * n));
    if (angles) {
        hipError_t e = gf_cached_malloc((void**)&d_ang, sizeof(double) * 4 * n);
        if (e != hipSuccess) { (void)gf_cached_free(d_fr); return gf_hip_fail(e, "hipMalloc(angles)"); }
    }
    int rc = gf_haar_draw_device(m, seed, first_draw, n, d_ang, d_fr);
    hipError_t e = hipSuccess;
    if (rc == GF_OK) e = hipMemcpyAsync(fr, d_fr, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, m->stream);
    if (rc == GF_OK && e == hipSuccess && angles)
        e = hipMemcpyAsync(angles, d_ang, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    (void)gf_cached_free(d_fr);
    if (d_ang) (void)gf_cached_free(d_ang);
    if (rc != GF_OK) return rc;
    return e != hipSuccess ? gf_hip_fail(e, "gf_haar_draw") : GF_OK;
}

// ---- device-resident entry points ----------------------------------------------------------
int gf_device_alloc(gf_model* m, size_t bytes, void** dptr)
{
    if (!m || !dptr) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(m->device));
    GF_HIP(gf_cached_malloc(dptr, bytes ? bytes : 16));
    return GF_OK;
}

int gf_device_free(gf_model* m, void* dptr)
{
    if (!m) return GF_ERR_INVALID_ARG;
    if (!dptr) return GF_OK;
    GF_HIP(hipSetDevice(m->device));
    if (m->stream) GF_HIP(hipStreamSynchronize(m->stream));
    GF_HIP(gf_cached_free(dptr));
    return GF_OK;
}

int gf_memcpy_h2d(gf_model* m, void* dst_dev, const void* src_host, size_t bytes)
{
    if (!m || !dst_dev || !src_host) return GF_ERR_INVALID_ARG;
    GF_STREAM(m);
    GF_HIP(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, m->stream));
    GF_HIP(hipStreamSynchronize(m->stream));
    return GF_OK;
}

int gf_memcpy_d2h(gf_model* m, void* dst_host, const void* src_dev, size_t bytes)
{
    if (!m || !dst_host || !src_dev) return GF_ERR_INVALID_ARG;
    GF_STREAM(m);
    return gf_internal_d2h(m->device, (void*)m->stream, dst_host, src_dev, bytes);
}

// the two device-resident batches
static int run_device(gf_model* m, const double* d_theta, int layout, int64_t n, double* d_lnprob, double* d_fr, int32_t* d_status, bool with_llh)
{
    if (!m || n < 0 || (layout != GF_LAYOUT_AOS && layout != GF_LAYOUT_SOA)) return GF_ERR_INVALID_ARG;
    if (n == 0) return GF_OK;
    int rc = check_dev_ptr(d_theta, 16);
    if (rc == GF_OK) rc = check_dev_ptr(with_llh ? d_lnprob : d_fr, 8);
    if (rc != GF_OK) return rc;
    GF_STREAM(m);
    std::lock_guard<std::mutex> lk(m->call_mu);
    return with_llh ? launch_lnprob(m, m->stream, d_theta, layout, n, d_lnprob, d_fr, d_status)
                    : launch_propagate(m, m->stream, d_theta, layout, n, d_fr, d_status);
}

int gf_lnprob_batch_device(gf_model* m, const double* d_theta, int layout, int64_t n, double* d_lnprob, double* d_fr,
                           int32_t* d_status)
{
    return run_device(m, d_theta, layout, n, d_lnprob, d_fr, d_status, true);
}

int gf_propagate_batch_device(gf_model* m, const double* d_theta, int layout, int64_t n, double* d_fr,
                              int32_t* d_status)
{
    return run_device(m, d_theta, layout, n, nullptr, d_fr, d_status, false);
}

int gf_haar_draw_device(gf_model* m, uint64_t seed, int64_t first_draw, int64_t n, double* d_angles, double* d_fr)
{
    if (!m || n < 0 || first_draw < 0) return GF_ERR_INVALID_ARG;
    if (n == 0) return GF_OK;
    int rc = check_dev_ptr(d_fr, 8);
    if (rc == GF_OK && d_angles) rc = check_dev_ptr(d_angles, 32);
    if (rc != GF_OK) return rc;
    GF_STREAM(m);
    hipError_t e = gf_launch_haar(m->c, seed, first_draw, n, d_angles, d_fr, m->cus, m->stream);
    return e != hipSuccess ? gf_hip_fail(e, "haar launch") : GF_OK;
}

// counts[nb][nb][nb] += histogram of n compositions resident on the device (asynchronous)
int gf_flavor_histogram_device(gf_model* m, const double* d_fr, int64_t n, int nbins, uint64_t* d_counts)
{
    if (!m || n < 0 || nbins < 1 || nbins > 1024) return GF_ERR_INVALID_ARG;
    if (n == 0) return GF_OK;
    int rc = check_dev_ptr(d_fr, 8);
    if (rc == GF_OK) rc = check_dev_ptr(d_counts, 8);
    if (rc != GF_OK) return rc;
    GF_STREAM(m);
    hipError_t e = gf_launch_flavor_hist(d_fr, n, nbins, (unsigned long long*)d_counts, m->cus, m->stream);
    return e != hipSuccess ? gf_hip_fail(e, "histogram launch") : GF_OK;
}

// host convenience: fr [n][3] -> counts [nbins]^3 (zeroed first)
int gf_flavor_histogram(gf_model* m, const double* fr, int64_t n, int nbins, uint64_t* counts)
{
    if (!m || n < 0 || (n > 0 && !fr) || !counts || nbins < 1 || nbins > 1024) return GF_ERR_INVALID_ARG;
    GF_STREAM(m);
    const size_t nbin3 = (size_t)nbins * nbins * nbins;
    double* d_fr = nullptr;
    uint64_t* d_c = nullptr;
    GF_HIP(gf_cached_malloc((void**)&d_c, sizeof(uint64_t) * nbin3));
    hipError_t e = hipMemsetAsync(d_c, 0, sizeof(uint64_t) * nbin3, m->stream);
    if (e == hipSuccess && n > 0) e = gf_cached_malloc((void**)&d_fr, sizeof(double) * 3 * n);
    if (e == hipSuccess && n > 0) e = hipMemcpyAsync(d_fr, fr, sizeof(double) * 3 * n, hipMemcpyHostToDevice, m->stream);
    int rc = GF_OK;
    if (e == hipSuccess && n > 0) rc = gf_flavor_histogram_device(m, d_fr, n, nbins, d_c);
    if (e == hipSuccess && rc == GF_OK) e = hipMemcpyAsync(counts, d_c, sizeof(uint64_t) * nbin3, hipMemcpyDeviceToHost, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    if (d_fr) (void)gf_cached_free(d_fr);
    (void)gf_cached_free(d_c);
    if (rc != GF_OK) return rc;
    return e != hipSuccess ? gf_hip_fail(e, "gf_flavor_histogram") : GF_OK;
}

int gf_model_sync(gf_model* m)
{
    if (!m) return GF_ERR_INVALID_ARG;
    if (!m->stream) return GF_OK;                               // no stream yet: nothing was ever enqueued
    GF_HIP(hipStreamSynchronize(m->stream));
    return check_queue_overflow(m->device, m->stream);          // of the *_device launches this call waited for
}

// internal, test hook (tests/test_gpu_unitarity_r3.py): the emulated-x87 unitarity residual (fr.py:489-494) of explicit
// (walker, bin) pairs of a device-resident theta block; which = 0: the serial chain of gf_x87.hpp (one lane per pair), 1: its
// three-lane distribution (what k_uni_resolve runs).  All pointers are device pointers; synchronous.
int gf_internal_uni_residuals(gf_model* m, const double* d_theta, int layout, int64_t n, const int64_t* d_walkers, const int32_t* d_bins,
                              int64_t npairs, int which, double* d_out)
{
    if (!m || !d_theta || !d_walkers || !d_bins || !d_out || m->c.mode != GF_MODE_BSM_GAUSS) return GF_ERR_INVALID_ARG;
    GF_STREAM(m);
    const hipError_t e = gf_launch_uni_debug(m->d_common, m->d_bsm, d_theta, layout, n, d_walkers, d_bins, npairs, which, d_out, m->stream);
    if (e != hipSuccess) return gf_hip_fail(e, "uni debug launch");
    GF_HIP(hipStreamSynchronize(m->stream));
    return GF_OK;
}

// internal, test hook (tests/test_gpu_x87_device.py): the primitives of gf_x87.hpp on device arrays (k_x87_eval, gf_unitarity.hip).
// op 0-3, 8: a, b -> one pair; 4, 6, 7: a -> one pair; 5: a -> two pairs; 9: n doubles ahi -> ohi; 10: 4 n doubles ahi -> 18 n pairs.
// All arrays are device pointers; synchronous.
int gf_internal_x87_eval(int device, int op, int64_t n, const double* d_ahi, const double* d_alo, const double* d_bhi, const double* d_blo,
                         double* d_ohi, double* d_olo)
{
    if (op < 0 || op > 10 || n < 0 || !d_ahi || !d_ohi) return GF_ERR_INVALID_ARG;
    if (op != 9 && op != 10 && !d_alo) return GF_ERR_INVALID_ARG;
    if (op != 9 && !d_olo) return GF_ERR_INVALID_ARG;
    if ((op <= 3 || op == 8) && (!d_bhi || !d_blo)) return GF_ERR_INVALID_ARG;
    if (n == 0) return GF_OK;
    int cus = 0;
    const int rc = pool_device(device, &cus);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(device));
    hipStream_t st = nullptr;
    GF_HIP(pool_stream(device, &st));
    const bool two = op <= 3 || op == 8;
    hipError_t e = gf_launch_x87_eval(op, n, d_ahi, d_alo, two ? d_bhi : nullptr, two ? d_blo : nullptr, d_ohi, d_olo, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    pool_release(device, st, nullptr);
    return e != hipSuccess ? gf_hip_fail(e, "x87 eval") : GF_OK;
}

int gf_event_create(void** ev)
{
    if (!ev) return GF_ERR_INVALID_ARG;
    hipEvent_t e;
    GF_HIP(hipEventCreate(&e));
    *ev = (void*)e;
    return GF_OK;
}

int gf_event_destroy(void* ev)
{
    if (!ev) return GF_OK;
    GF_HIP(hipEventDestroy((hipEvent_t)ev));
    return GF_OK;
}

int gf_event_record(gf_model* m, void* ev)
{
    if (!m || !ev) return GF_ERR_INVALID_ARG;
    GF_STREAM(m);
    GF_HIP(hipEventRecord((hipEvent_t)ev, m->stream));
    return GF_OK;
}

int gf_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms)
{
    if (!ev_start || !ev_stop || !ms) return GF_ERR_INVALID_ARG;
    GF_HIP(hipEventSynchronize((hipEvent_t)ev_stop));
    GF_HIP(hipEventElapsedTime(ms, (hipEvent_t)ev_start, (hipEvent_t)ev_stop));
    return GF_OK;
}

}  // extern "C"
