// prof.h -- per-kernel timing with pairs of HIP events, for the handles that offer a profile (hipts_vit_profile_*, hipts_query_profile_*).
// A Scope around a launch records an event before and after it on the launch's stream; resolve() waits for the pairs recorded so far
// and adds their times, flops and bytes to the totals of their category.  Events are recycled, never created on a warm path.
#pragma once
#include <vector>

#include "common.h"

namespace hipts {
#pragma GCC visibility push(hidden)      // internal: nothing here joins the library's exported symbols
template <int NCAT>
struct EventProfile {
    struct Rec { int cat; hipEvent_t a, b; double flops, bytes; };
    std::vector<Rec> recs;              // recorded, not yet resolved
    std::vector<hipEvent_t> pool;       // recycled events
    double ms[NCAT] = {0}, flops[NCAT] = {0}, bytes[NCAT] = {0};
    int64_t n[NCAT] = {0};

    hipEvent_t get() {                  // a recycled event or a new one; nullptr when none can be created
        hipEvent_t e = nullptr;
        if (pool.empty()) return hipEventCreate(&e) == hipSuccess ? e : nullptr;
        e = pool.back();
        pool.pop_back();
        return e;
    }
    // RAII around the launches of category `cat` on stream s; p == nullptr: not recorded
    struct Scope {
        EventProfile* p;
        hipStream_t s;
        Rec r{};
        Scope(EventProfile* p_, hipStream_t s_, int cat, double flops_, double bytes_) : p(p_), s(s_) {
            if (!p) return;
            r = Rec{cat, p->get(), p->get(), flops_, bytes_};
            if (r.a) (void)hipEventRecord(r.a, s);
        }
        ~Scope() {
            if (!p) return;
            if (r.b) (void)hipEventRecord(r.b, s);
            p->recs.push_back(r);
        }
    };
    // the unresolved records' events go back to the pool, their measurements are dropped
    void recycle() {
        for (auto& r : recs)
            for (hipEvent_t e : {r.a, r.b})
                if (e) pool.push_back(e);
        recs.clear();
    }
    // a new measurement window: totals zero, nothing recorded before it counts
    void reset() {
        recycle();
        for (int c = 0; c < NCAT; ++c) ms[c] = flops[c] = bytes[c] = n[c] = 0;
    }
    // waits for every recorded pair and adds it to its category's totals
    int resolve() {
        for (auto& r : recs) {
            if (!r.a || !r.b) continue;
            HIPTS_HIP(hipEventSynchronize(r.b));
            float t = 0.f;
            HIPTS_HIP(hipEventElapsedTime(&t, r.a, r.b));
            ms[r.cat] += t;
            n[r.cat] += 1;
            flops[r.cat] += r.flops;
            bytes[r.cat] += r.bytes;
        }
        recycle();
        return HIPTS_OK;
    }
    ~EventProfile() {                   // the owning handle's destroy function has selected the device
        recycle();
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    }
};
#pragma GCC visibility pop
}  // namespace hipts
