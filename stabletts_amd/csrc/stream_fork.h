// Fork / join of engine-owned child streams (engine_dit.h: DitState::part_streams, engine_train.cpp: TrainState::side*).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

namespace sthost {

// Work forked from a parent stream onto engine-owned child streams and joined back with events: the only place the engine
// makes one stream wait for another.  fork() makes children 0 .. n-1 wait for everything queued on the parent so far (its events
// form a ring, one per fork); join() records each forked child's join event -- unless record_join() did, right after the child's
// last work -- makes the parent wait for it and clears the pending sites.  Sites (training): record_site(k) marks what child 0 has
// queued so far, wait_site(k, parent) makes the parent wait for that mark once.  Without child streams fork, join and the sites
// are no-ops and on() is the parent.  Errors are returned as the first failing HIP call's (callers wrap them in HIPCHK).
struct StreamFork {
    static constexpr int kMaxChildren = 3, kMaxRing = 16, kMaxSites = 12;      // (solve parts 1 .. 3; training: 16 fork events, 12 dY sites)
    hipStream_t child[kMaxChildren] = {};
    hipEvent_t ev_fork[kMaxRing] = {}, ev_join[kMaxChildren] = {}, ev_site[kMaxSites] = {};
    bool site_pending[kMaxSites] = {}, join_recorded = false;
    int n = 0, ring = 0, fork_idx = 0, forked = 0;      // forked: children forked since the last join

    // creates what is missing of `ring_` fork events, `children` streams (at `priority` if given) with their join events, `sites` site events
    hipError_t ensure(int children, int ring_, int sites, const int* priority = nullptr) {
        hipError_t r;
        for (; ring < ring_; ++ring) if ((r = hipEventCreateWithFlags(&ev_fork[ring], hipEventDisableTiming))) return r;
        for (; n < children; ++n) {
            r = priority ? hipStreamCreateWithPriority(&child[n], hipStreamNonBlocking, *priority) : hipStreamCreateWithFlags(&child[n], hipStreamNonBlocking);
            if (r || (r = hipEventCreateWithFlags(&ev_join[n], hipEventDisableTiming))) return r;
        }
        for (int k = 0; k < sites; ++k) if (!ev_site[k] && (r = hipEventCreateWithFlags(&ev_site[k], hipEventDisableTiming))) return r;
        return hipSuccess;
    }
    void destroy() {        // synchronises and destroys the streams, destroys the events
        for (int k = 0; k < n; ++k) { hipStreamSynchronize(child[k]); hipStreamDestroy(child[k]); }
        for (hipEvent_t ev : ev_fork) if (ev) hipEventDestroy(ev);
        for (hipEvent_t ev : ev_join) if (ev) hipEventDestroy(ev);
        for (hipEvent_t ev : ev_site) if (ev) hipEventDestroy(ev);
        *this = StreamFork();
    }
    hipStream_t on(hipStream_t parent) const { return n ? child[0] : parent; }
    hipError_t fork(hipStream_t parent, int children = 1) {
        children = std::min(children, n);
        if (children == 0) return hipSuccess;
        forked = std::max(forked, children);
        const hipEvent_t f = ev_fork[fork_idx]; fork_idx = (fork_idx + 1) % ring;
        hipError_t r = hipEventRecord(f, parent);
        for (int k = 0; r == hipSuccess && k < children; ++k) r = hipStreamWaitEvent(child[k], f, 0);
        return r;
    }
    hipError_t record_join() {
        hipError_t r = hipSuccess;
        for (int k = 0; r == hipSuccess && k < forked; ++k) r = hipEventRecord(ev_join[k], child[k]);
        join_recorded = r == hipSuccess;
        return r;
    }
    hipError_t join(hipStream_t parent) {        // tries every child whatever fails: the first error is returned
        hipError_t first = hipSuccess;
        for (int k = 0; k < forked; ++k) {
            hipError_t r = join_recorded ? hipSuccess : hipEventRecord(ev_join[k], child[k]);
            if (r == hipSuccess) r = hipStreamWaitEvent(parent, ev_join[k], 0);
            if (first == hipSuccess) first = r;
        }
        forked = 0; join_recorded = false;
        for (bool& p : site_pending) p = false;
        return first;
    }
    hipError_t record_site(int k) {
        if (n == 0) return hipSuccess;
        const hipError_t r = hipEventRecord(ev_site[k], child[0]);
        site_pending[k] = r == hipSuccess;
        return r;
    }
    hipError_t wait_site(int k, hipStream_t parent) {
        if (!site_pending[k]) return hipSuccess;
        site_pending[k] = false;
        return hipStreamWaitEvent(parent, ev_site[k], 0);
    }
};

// Joins a StreamFork that is still forked when the scope is left: an early error return between fork and join must not hand the
// parent stream back while the children still run.  Best effort: its own HIP errors are ignored, the call keeps its first error.
struct ForkGuard {
    StreamFork& f; hipStream_t parent;
    ~ForkGuard() { if (f.forked) (void)f.join(parent); }
};

}  // namespace sthost
