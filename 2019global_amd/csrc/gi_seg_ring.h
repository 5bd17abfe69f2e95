// gi_seg_ring.h — the wave-uniform unit accounting of k_seg (gi_wf.hip): which (pixel, sample) units a
// wave owns, which of them it has generated, and how many prepared primary rays wait in its LDS ring.
// Host and device: the kernel calls these functions, and tests/cpp/seg_ring_check.cpp drives the same
// functions for simulated waves on the CPU.
//
// A wave owns the units [cur, cur_end) of its current run; a run is `run` units taken from the
// launch's one counter with one atomic (give_run).  With the ring, units leave the run a batch at a
// time (take_batch: the next <= 64 of the run), every lane of the wave generates one unit of the batch,
// and the primary rays that hit the scene's root box are parked in the ring (push) until lanes whose
// path has ended take them (pop).  A batch is generated only into an empty ring, so the ring's entries
// are always the slots [head, head + count) of 64 and never wrap.
#ifndef GI_SEG_RING_H_
#define GI_SEG_RING_H_

#include "gi_math.h"

namespace gi {

constexpr unsigned kSegBatch = 64;   // units per batch: one per lane of the wave

struct SegUnits {
    unsigned long long cur = 0, cur_end = 0;   // the wave's unhanded units [cur, cur_end)
    bool exhausted = false;                    // the launch's units are all handed out to some wave
    unsigned head = 0, count = 0;              // the ring's entries: slots [head, head + count)

    // units that no lane has generated yet may still come: from the wave's run or from the counter
    GI_HD bool units_left() const { return !(exhausted && cur >= cur_end); }
    // the wave's part of the launch is finished (the kernel's loop ends when also no lane is live)
    GI_HD bool done() const { return !units_left() && count == 0; }
    // a batch is due: some lane needs a ray, the ring has none, and units remain
    GI_HD bool wants_batch(unsigned n_need) const { return n_need != 0 && count == 0 && units_left(); }
    // ... and it needs a fresh run from the counter first
    GI_HD bool wants_run() const { return cur >= cur_end && !exhausted; }
    // the counter's answer nb (its value before this wave added `run`) for a launch of `total` units
    GI_HD void give_run(unsigned long long nb, unsigned long long run, unsigned long long total) {
        if (nb >= total) {
            exhausted = true;
        } else {
            cur = nb;
            cur_end = nb + run < total ? nb + run : total;
            if (cur_end == total) exhausted = true;
        }
    }
    // the next batch of the run: units [first, first + n), n <= 64 (0: the launch has no unit left)
    GI_HD unsigned take_batch(unsigned long long& first) {
        const unsigned long long left = cur_end > cur ? cur_end - cur : 0ull;
        const unsigned n = left < kSegBatch ? (unsigned)left : kSegBatch;
        first = cur;
        cur += n;
        return n;
    }
    // the batch's n_hit prepared rays now fill the slots [0, n_hit) of the (empty) ring
    GI_HD void push(unsigned n_hit) {
        head = 0;
        count = n_hit;
    }
    // n_need lanes ask: the first k of them (by rank) take the slots first .. first + k - 1
    GI_HD unsigned pop(unsigned n_need, unsigned& first) {
        const unsigned k = n_need < count ? n_need : count;
        first = head;
        head += k;
        count -= k;
        return k;
    }
};

}  // namespace gi

#endif  // GI_SEG_RING_H_
