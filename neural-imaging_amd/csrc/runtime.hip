// Host code only - the library's process-wide state and its stream helpers in one place: the ABI version, the per-stream
// bindings of the split-K arrival counters (behind a mutex), and streams restricted to a number of compute units.
#include <stdlib.h>
#include <mutex>

#include "common.h"

extern "C" {

int nimg_abi_version(void) { return NIMG_ABI_VERSION; }

// ---- arrival counters of the in-kernel split-K finish (common.h ticket_finish): caller-owned zeroed device memory per stream
namespace {
struct TicketBinding { hipStream_t stream; unsigned* buf; size_t words; bool used; };
TicketBinding g_tickets[NIMG_TICKET_STREAMS];
std::mutex g_tickets_mutex;
}  // namespace

int nimg_bind_tickets(void* stream, void* buf, size_t bytes) {
    if ((buf && (bytes < 4 || (bytes & 3))) || ((uintptr_t)buf & 3)) return NIMG_ERR_ARG;
    std::lock_guard<std::mutex> lock(g_tickets_mutex);
    int free_slot = -1;
    for (int i = 0; i < NIMG_TICKET_STREAMS; ++i) {
        if (g_tickets[i].used && g_tickets[i].stream == (hipStream_t)stream) {
            if (buf) { g_tickets[i].buf = (unsigned*)buf; g_tickets[i].words = bytes / 4; }
            else g_tickets[i].used = false;
            return NIMG_OK;
        }
        if (!g_tickets[i].used && free_slot < 0) free_slot = i;
    }
    if (!buf) return NIMG_OK;
    if (free_slot < 0) return NIMG_ERR_ARG;
    g_tickets[free_slot] = TicketBinding{(hipStream_t)stream, (unsigned*)buf, bytes / 4, true};
    return NIMG_OK;
}

int nimg_stream_create_cu_mask(int n_cus, void** stream) {
    if (!stream || n_cus < 1 || n_cus > 1024) return NIMG_ERR_ARG;
    uint32_t mask[32] = {0};
    for (int i = 0; i < n_cus; ++i) mask[i >> 5] |= 1u << (i & 31);
    hipStream_t s = nullptr;
    if (hipExtStreamCreateWithCUMask(&s, (uint32_t)((n_cus + 31) / 32), mask) != hipSuccess) return NIMG_ERR_LAUNCH;
    *stream = (void*)s;
    return NIMG_OK;
}

int nimg_stream_destroy(void* stream) {
    if (!stream) return NIMG_ERR_ARG;
    return hipStreamDestroy((hipStream_t)stream) == hipSuccess ? NIMG_OK : NIMG_ERR_LAUNCH;
}

unsigned* nimg_internal_tickets(hipStream_t stream, size_t words) {
    static const bool off = getenv("NIMG_NO_TICKETS") != nullptr;
    if (off) return nullptr;
    std::lock_guard<std::mutex> lock(g_tickets_mutex);
    for (int i = 0; i < NIMG_TICKET_STREAMS; ++i)
        if (g_tickets[i].used && g_tickets[i].stream == stream) return g_tickets[i].words >= words ? g_tickets[i].buf : nullptr;
    return nullptr;
}

}  // extern "C"
