// zlz4_host.hip -- the per-process state behind zlz4_host.hpp: the device probe and the parked-buffer cache.  Host code
// only.
#include "zlz4_host.hpp"

#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/zlz4_amd.h"

namespace {

// ---------------------------------------------------------------- parked device buffers
struct ParkedBuf { void *p; size_t n; int dev; };
std::mutex g_park_mutex;
std::vector<ParkedBuf> g_parked;
size_t g_parked_bytes = 0;
constexpr size_t kMaxParked = 12;
constexpr size_t kMaxParkedBytes = 8ull << 30;   // ~3 % of the HBM: one configs[4] slot arena (4 GiB) and its tables

}  // namespace

namespace zlz4host {

bool device_ok() {
    static const bool ok = [] {
        int n = 0, dev = 0;
        hipDeviceProp_t p;
        return hipGetDeviceCount(&n) == hipSuccess && n > 0 && hipGetDevice(&dev) == hipSuccess &&
               hipGetDeviceProperties(&p, dev) == hipSuccess &&
               std::strncmp(p.gcnArchName, "gfx950", 6) == 0;      // kernels are built for gfx950 only
    }();
    return ok;
}

void *cache_take(size_t &n, int dev) {
    std::lock_guard<std::mutex> lock(g_park_mutex);
    size_t best = g_parked.size();
    for (size_t i = 0; i < g_parked.size(); i++)     // smallest parked buffer that fits and is not wastefully large
        if (g_parked[i].dev == dev && g_parked[i].n >= n && g_parked[i].n / 2 <= n + (1u << 20) &&
            (best == g_parked.size() || g_parked[i].n < g_parked[best].n))
            best = i;
    if (best == g_parked.size()) return nullptr;
    void *p = g_parked[best].p;
    n = g_parked[best].n;
    g_parked_bytes -= n;
    g_parked.erase(g_parked.begin() + (long)best);
    return p;
}

bool cache_give(void *p, size_t n, int dev) {
    std::lock_guard<std::mutex> lock(g_park_mutex);
    if (g_parked.size() >= kMaxParked || g_parked_bytes + n > kMaxParkedBytes) return false;
    g_parked.push_back({p, n, dev});
    g_parked_bytes += n;
    return true;
}

}  // namespace zlz4host

extern "C" void zlz4_release_device_cache(void) {
    std::vector<ParkedBuf> take;
    {
        std::lock_guard<std::mutex> lock(g_park_mutex);
        take.swap(g_parked);
        g_parked_bytes = 0;
    }
    for (const ParkedBuf &b : take) (void)hipFree(b.p);
}
