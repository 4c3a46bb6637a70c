// sdrk_api.hip — the base of the host side of the C ABI declared in include/sdrk.h: error reporting, device queries and
// plain device memory, the table of pinned host ranges, device staging that only grows.  The other host files (sdrk_plan.hip,
// sdrk_host_pipeline.hip, sdrk_features.hip, sdrk_waterfall.hip, sdrk_probes.hip, sdrk_f64.hip) build on it through
// plan_internal.h.  All compute is in the gfx950 kernels; there is no host fallback in any of these files.
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <string>

#include "host_pool.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace sdrk_host {

namespace {
thread_local std::string g_last_error = "";
}  // namespace

int fail(int status, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return status;
}

int check_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(SDRK_ERR_NO_DEVICE, "no HIP device available (%s)",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    }
    if (device < 0 || device >= n)
        return fail(SDRK_ERR_NO_DEVICE, "device %d out of range (%d visible)", device, n);
    return SDRK_OK;
}

bool is_pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }

PinnedRanges& pinned_ranges() {
    static PinnedRanges pr;
    return pr;
}

// Device staging that only ever grows (no free + malloc per call once the largest size has been seen).
int grow(int device, void** buf, size_t* cap, size_t need) {
    if (need <= *cap) return SDRK_OK;
    if (*buf) {
        HIP_TRY(hipFree(*buf));
        *buf = nullptr;
        *cap = 0;
    }
    const size_t want = need + need / 4;   // head-room: a slightly larger next call does not reallocate
    if (hipMalloc(buf, want) != hipSuccess) {
        (void)hipGetLastError();
        HIP_TRY(hipMalloc(buf, need));
        *cap = need;
    } else {
        *cap = want;
    }
    (void)device;
    return SDRK_OK;
}

}  // namespace sdrk_host

extern "C" {

int sdrk_version(void) { return SDRK_VERSION; }

const char* sdrk_last_error(void) { return g_last_error.c_str(); }

int sdrk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int sdrk_device_info(int device, char* buf, size_t buf_len) {
    if (!buf || buf_len == 0) return fail(SDRK_ERR_INVALID, "buf is NULL/empty");
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    snprintf(buf, buf_len, "%s %s, %d CUs, %.1f GiB, %d MHz, pci %04x:%02x:%02x.0", prop.gcnArchName, prop.name,
             prop.multiProcessorCount, (double)prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0),
             prop.clockRate / 1000, prop.pciDomainID, prop.pciBusID, prop.pciDeviceID);
    return SDRK_OK;
}

int sdrk_dev_alloc(int device, size_t bytes, void** d_ptr) {
    if (!d_ptr) return fail(SDRK_ERR_INVALID, "d_ptr is NULL");
    *d_ptr = nullptr;
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(d_ptr, bytes ? bytes : 1));
    return SDRK_OK;
}

int sdrk_dev_mem_info(int device, size_t* free_bytes, size_t* total_bytes) {
    if (!free_bytes || !total_bytes) return fail(SDRK_ERR_INVALID, "free_bytes / total_bytes is NULL");
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemGetInfo(free_bytes, total_bytes));
    return SDRK_OK;
}

int sdrk_dev_free(int device, void* d_ptr) {
    if (!d_ptr) return SDRK_OK;
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(d_ptr));
    return SDRK_OK;
}

int sdrk_memcpy_h2d(int device, void* d_dst, const void* h_src, size_t bytes) {
    if (bytes == 0) return SDRK_OK;
    if (!d_dst || !h_src) return fail(SDRK_ERR_INVALID, "NULL pointer");
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return SDRK_OK;
}

int sdrk_memcpy_d2h(int device, void* h_dst, const void* d_src, size_t bytes) {
    if (bytes == 0) return SDRK_OK;
    if (!h_dst || !d_src) return fail(SDRK_ERR_INVALID, "NULL pointer");
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return SDRK_OK;
}

int sdrk_host_alloc(size_t bytes, void** h_ptr) {
    if (!h_ptr) return fail(SDRK_ERR_INVALID, "h_ptr is NULL");
    *h_ptr = nullptr;
    if (bytes == 0) return fail(SDRK_ERR_INVALID, "bytes must be >= 1");
    int st = check_device(0);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipHostMalloc(h_ptr, bytes, hipHostMallocPortable));
    std::lock_guard<std::mutex> g(pinned_ranges().m);
    pinned_ranges().r[reinterpret_cast<uintptr_t>(*h_ptr)] = {bytes, true};
    return SDRK_OK;
}

int sdrk_host_free(void* h_ptr) {
    if (!h_ptr) return SDRK_OK;
    {
        std::lock_guard<std::mutex> g(pinned_ranges().m);
        auto it = pinned_ranges().r.find(reinterpret_cast<uintptr_t>(h_ptr));
        if (it == pinned_ranges().r.end() || !it->second.second)
            return fail(SDRK_ERR_INVALID, "pointer was not returned by sdrk_host_alloc");
        pinned_ranges().r.erase(it);
    }
    HIP_TRY(hipHostFree(h_ptr));
    return SDRK_OK;
}

int sdrk_host_register(void* h_ptr, size_t bytes) {
    if (!h_ptr || bytes == 0) return fail(SDRK_ERR_INVALID, "NULL pointer or zero bytes");
    int st = check_device(0);
    if (st != SDRK_OK) return st;
    {
        std::lock_guard<std::mutex> g(pinned_ranges().m);
        if (pinned_ranges().r.count(reinterpret_cast<uintptr_t>(h_ptr)))
            return fail(SDRK_ERR_INVALID, "range is already registered");
    }
    HIP_TRY(hipHostRegister(h_ptr, bytes, hipHostRegisterPortable));
    std::lock_guard<std::mutex> g(pinned_ranges().m);
    pinned_ranges().r[reinterpret_cast<uintptr_t>(h_ptr)] = {bytes, false};
    return SDRK_OK;
}

int sdrk_host_unregister(void* h_ptr) {
    if (!h_ptr) return SDRK_OK;
    {
        std::lock_guard<std::mutex> g(pinned_ranges().m);
        auto it = pinned_ranges().r.find(reinterpret_cast<uintptr_t>(h_ptr));
        if (it == pinned_ranges().r.end() || it->second.second)
            return fail(SDRK_ERR_INVALID, "pointer was not registered with sdrk_host_register");
        pinned_ranges().r.erase(it);
    }
    HIP_TRY(hipHostUnregister(h_ptr));
    return SDRK_OK;
}

int sdrk_host_is_pinned(const void* h_ptr, size_t bytes) { return pinned_ranges().covers(h_ptr, bytes) ? 1 : 0; }

int sdrk_host_threads(void) { return sdrk::CopyPool::get().helpers(); }

}  // extern "C"
