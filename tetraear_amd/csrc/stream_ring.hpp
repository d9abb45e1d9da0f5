// Slot bookkeeping of tdm_stream (include/tetrahip.h): host only, no HIP, so that a CPU test can compile it alone and
// drive it.  A ring of `depth` slots; step `seq` uses slot seq % depth.  A slot is FREE (its last result collected, or never
// used), FILLING (acquired: the caller writes its page-locked input) or IN_FLIGHT (submitted, result not collected yet).
// Results are collected in submission order, and a slot is handed out again only after its result was collected, so at
// most `depth` steps are outstanding and the host memory a result points into stays put until its slot is acquired again.
// Every transition is two-phase: the query names the slot, the commit happens only after the device work for it was
// enqueued (submit) or waited for (collect) -- a call that fails in between leaves the ring as it was.
#pragma once

#include <cstdint>
#include <vector>

namespace tdm {

struct StreamRing {
    enum State { FREE = 0, FILLING = 1, IN_FLIGHT = 2 };
    std::vector<State> st;
    int64_t next_submit = 0;    // seq of the next step to be submitted (the acquired one, if a slot is FILLING)
    int64_t next_collect = 0;   // seq of the oldest step not collected yet
    int filling = -1;           // the acquired slot, or -1

    explicit StreamRing(int depth = 1) : st((size_t)(depth > 0 ? depth : 1), FREE) {}
    int depth() const { return (int)st.size(); }
    int64_t in_flight() const { return next_submit - next_collect; }

    // 0: *slot / *seq name the slot to fill (the same one again if it is acquired already); -1: refused, *why says why
    int acquire(int *slot, int64_t *seq, const char **why)
    {
        const int k = (int)(next_submit % depth());
        if (filling < 0 && st[k] == IN_FLIGHT) {
            *why = "tdm_stream_acquire: the next slot still holds an uncollected result (collect the oldest step first)";
            return -1;
        }
        filling = k;
        st[k] = FILLING;
        *slot = k;
        *seq = next_submit;
        return 0;
    }
    // the slot a submit goes to, or -1 (nothing acquired)
    int submit_slot() const { return filling; }
    void commit_submit()
    {
        st[filling] = IN_FLIGHT;
        filling = -1;
        ++next_submit;
    }
    // the slot of the oldest uncollected step, or -1 (nothing in flight)
    int collect_slot() const
    {
        if (next_collect == next_submit) return -1;
        return (int)(next_collect % depth());
    }
    void commit_collect()
    {
        st[(size_t)(next_collect % depth())] = FREE;
        ++next_collect;
    }
};

}  // namespace tdm
