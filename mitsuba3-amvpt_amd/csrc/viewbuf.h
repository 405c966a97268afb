/*
 * viewbuf.h -- the uploads of a view table, for the units whose kernels read one (amvpt_temporal.hip, amvpt_synth.hip).
 * A ViewBuf is a device buffer with a pinned host block of the same size.  A call takes a kept ViewBuf of its device
 * that is large enough and whose last use has finished (the event behind that launch, polled: nobody waits), or
 * allocates one; it copies the caller's table into the pinned block before it returns, so the caller's memory, pageable
 * or pinned, is free again and the copy to the device is asynchronous; it records the event behind its own launch and
 * gives the ViewBuf back.  Calls on several streams never share one in flight.  Limits (also in the headers): the pool
 * does not shrink -- it holds as many ViewBufs as calls were ever enqueued at once, whole 4 KiB of each memory and one
 * event apiece -- and a call that has to allocate cannot be captured into a graph.
 * view_buf_launch is that whole sequence around a caller's fill and launch.
 * Every unit that includes this has a pool of its own (the state below is static): the units share the code, no state.
 * `who` is the entry's name, the first word of every message.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <mutex>
#include <string>
#include <vector>

#include "internal.h"

namespace amvpt {

struct ViewBuf {
    void *p = nullptr;      /* device */
    void *host = nullptr;   /* pinned */
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    int device = 0;
};
static std::mutex g_view_mutex;
static std::vector<ViewBuf> g_view_bufs;

static amvpt_status view_buf_take(const std::string &who, size_t bytes, ViewBuf &b) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail((who + " hipGetDevice").c_str(), (int) e);
    {
        std::lock_guard<std::mutex> lock(g_view_mutex);
        for (size_t i = 0; i < g_view_bufs.size(); ++i) {
            const ViewBuf &c = g_view_bufs[i];
            if (c.device != dev || c.bytes < bytes || hipEventQuery(c.done) != hipSuccess) continue;
            b = c;
            g_view_bufs.erase(g_view_bufs.begin() + (ptrdiff_t) i);
            return AMVPT_OK;
        }
    }
    b = ViewBuf{};
    b.device = dev;
    b.bytes = (bytes + 4095u) & ~(size_t) 4095u;
    e = hipMalloc(&b.p, b.bytes);
    if (e != hipSuccess) { set_error(who + ": hipMalloc of the view table failed"); return AMVPT_ERR_OOM; }
    e = hipHostMalloc(&b.host, b.bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void) hipFree(b.p);
        set_error(who + ": hipHostMalloc of the view table's staging block failed");
        return AMVPT_ERR_OOM;
    }
    e = hipEventCreateWithFlags(&b.done, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void) hipFree(b.p);
        (void) hipHostFree(b.host);
        return hip_fail((who + " hipEventCreate").c_str(), (int) e);
    }
    return AMVPT_OK;
}
/* behind the launch (or the failed attempt) on `st` */
static hipError_t view_buf_give(const ViewBuf &b, hipStream_t st) {
    const hipError_t e = hipEventRecord(b.done, st);
    std::lock_guard<std::mutex> lock(g_view_mutex);
    g_view_bufs.push_back(b);
    return e;
}

/* a call's device half: fill(host block) writes the `bytes` of its table, which go up on `st`; launch(device block)
 * enqueues the kernel behind them and returns hipGetLastError(); the ViewBuf goes back behind that either way */
template <class Fill, class Launch>
static amvpt_status view_buf_launch(const std::string &who, size_t bytes, hipStream_t st, Fill fill, Launch launch) {
    ViewBuf vb;
    if (amvpt_status rc = view_buf_take(who, bytes, vb)) return rc;
    fill(vb.host);
    hipError_t e = hipMemcpyAsync(vb.p, vb.host, bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch((const void *) vb.p);
    const hipError_t eg = view_buf_give(vb, st);
    if (e != hipSuccess) return hip_fail((who + " launch").c_str(), (int) e);
    if (eg != hipSuccess) return hip_fail((who + " hipEventRecord").c_str(), (int) eg);
    return AMVPT_OK;
}

} // namespace amvpt
