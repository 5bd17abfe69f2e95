// CPU check of k_seg's unit accounting (2019global_amd/csrc/gi_seg_ring.h SegUnits: the functions the
// kernel itself calls).  Several simulated waves share one unit counter, as the waves of a launch share
// the device counter; each wave runs k_seg's loop -- refill from the ring, generating a batch into the
// empty ring when lanes need rays, then one "segment" after which a seeded random set of lanes has
// ended its path.  Which units miss the root box is a seeded random set too.
//
// Checked for totals of 0, 1, 63, 64, 65, 127, 128, 129 and 64 k + 1 units, runs of 64 and 128 units:
//   every unit in [0, total) is generated exactly once; every hit is popped exactly once, by a lane that
//   needed one, and no miss is ever popped; the ring never holds more than 64 entries and a pop never
//   reaches past the pushed ones; every wave terminates, with an empty ring and no live lane.
// Prints one line per configuration and "failures N" last; exit status 1 when N > 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gi_seg_ring.h"

namespace {

constexpr int kBurst = 16;   // GI_SEG_BURST

uint64_t mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
struct Rng {
    uint64_t s;
    uint64_t next() { return mix(s += 0x9E3779B97F4A7C15ull); }
    bool chance(unsigned per256) { return (next() & 255u) < per256; }
};

struct Wave {
    gi::SegUnits su;
    uint64_t live = 0;          // lanes that carry a path
    uint64_t ring[64] = {};     // the ring's entries: unit numbers
    bool finished = false;
    unsigned long long iters = 0;
};

struct Sim {
    unsigned long long total, run, counter = 0;
    unsigned miss256, die256;   // of 256: units that miss the root box, live lanes that end per segment
    uint64_t seed;
    std::vector<uint8_t> made, popped;
    long long failures = 0;

    bool misses(unsigned long long u) const { return (mix(seed ^ (u * 0x2545F4914F6CDD1Dull + 1)) & 255u) < miss256; }
    void fail(const char* what, unsigned long long v) {
        if (failures++ < 10) std::printf("  FAIL %s (%llu): total %llu run %llu miss %u die %u\n", what, v, total, run, miss256, die256);
    }

    // one iteration of k_seg's loop for wave w: true while the wave goes on
    bool iterate(Wave& w, Rng& rng) {
        ++w.iters;
        for (int burst = 0; burst < kBurst; ++burst) {
            const uint64_t m_need = ~w.live;
            if (m_need == 0 || w.su.done()) break;
            const unsigned n_need = (unsigned)__builtin_popcountll(m_need);
            if (w.su.wants_batch(n_need)) {
                if (w.su.count != 0) fail("batch into a ring that is not empty", w.su.count);
                if (w.su.wants_run()) {
                    const unsigned long long nb = counter;   // the atomic add
                    counter += run;
                    w.su.give_run(nb, run, total);
                }
                unsigned long long first = 0;
                unsigned n = w.su.take_batch(first);
                if (n > 64) {
                    fail("batch of more than 64 units", n);
                    n = 64;
                }
                unsigned n_hit = 0;
                for (unsigned lane = 0; lane < n; ++lane) {
                    const unsigned long long u = first + lane;
                    if (u >= total) { fail("unit beyond the launch", u); continue; }
                    if (made[u]++) fail("unit generated twice", u);
                    if (!misses(u)) w.ring[n_hit++] = u;
                }
                if (n != 0) w.su.push(n_hit);
                if (w.su.count > 64) fail("ring holds more than 64", w.su.count);
            }
            const unsigned before = w.su.count, head = w.su.head;
            unsigned first_e = 0;
            const unsigned k = w.su.pop(n_need, first_e);
            if (k > n_need || k > before) fail("pop hands out more than asked or held", k);
            if (first_e != head || first_e + k > 64) fail("pop outside the pushed entries", first_e + k);
            unsigned rank = 0;
            for (int lane = 0; lane < 64 && rank < k; ++lane) {
                if (w.live >> lane & 1) continue;
                const uint64_t u = w.ring[first_e + rank++];
                if (u >= total) { fail("popped entry is no unit", u); continue; }
                if (misses(u)) fail("a miss was popped", u);
                if (popped[u]++) fail("hit popped twice", u);
                w.live |= 1ull << lane;
            }
        }
        if (w.live == 0) return !w.su.done();
        // the segment: some paths end
        for (int lane = 0; lane < 64; ++lane)
            if ((w.live >> lane & 1) && rng.chance(die256)) w.live &= ~(1ull << lane);
        return true;
    }

    void run_all(int n_waves) {
        made.assign((size_t)total, 0);
        popped.assign((size_t)total, 0);
        std::vector<Wave> waves((size_t)n_waves);
        Rng rng{seed};
        const unsigned long long limit = 64 + 8 * (total + 64) * 256 / (die256 ? die256 : 1);
        int open = n_waves;
        while (open > 0) {
            Wave& w = waves[(size_t)(rng.next() % (uint64_t)n_waves)];   // the waves interleave at random
            if (w.finished) continue;
            if (!iterate(w, rng)) {
                w.finished = true;
                --open;
                if (w.su.count != 0 || !w.su.done()) fail("wave ended with entries in its ring", w.su.count);
                if (w.live != 0) fail("wave ended with live lanes", (unsigned long long)__builtin_popcountll(w.live));
            } else if (w.iters > limit) {
                fail("wave does not terminate", w.iters);
                return;
            }
        }
        for (unsigned long long u = 0; u < total; ++u) {
            if (made[u] != 1) fail("unit not generated exactly once", u);
            if (popped[u] != (misses(u) ? 0 : 1)) fail("hit not popped exactly once", u);
        }
    }
};

}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 4;
    const unsigned long long totals[] = {0, 1, 63, 64, 65, 127, 128, 129, 64 * 1024 + 1};
    const unsigned long long runs[] = {64, 128};
    const unsigned miss[] = {0, 64, 200, 256};   // none, a quarter, most, every unit misses the root box
    const unsigned die[] = {256, 54, 8};         // every lane ends every segment (depth 1), about a fifth, few
    const int waves[] = {1, 3, 16};
    long long failures = 0, configs = 0;
    for (unsigned long long total : totals)
        for (unsigned long long run : runs) {
            long long f = 0;
            for (unsigned ms : miss)
                for (unsigned di : die)
                    for (int nw : waves)
                        for (int r = 0; r < rounds; ++r) {
                            if (total > 1000 && r > 0) continue;   // the large total once per combination
                            Sim s{total, run};
                            s.miss256 = ms;
                            s.die256 = di;
                            s.seed = mix(total * 1315423911ull + run * 2654435761ull + ms * 97 + di * 13 + (unsigned)nw * 7 + (unsigned)r);
                            s.run_all(nw);
                            f += s.failures;
                            ++configs;
                        }
            std::printf("total %llu run %llu: failures %lld\n", total, run, f);
            failures += f;
        }
    std::printf("configurations %lld\n", configs);
    std::printf("failures %lld\n", failures);
    return failures ? 1 : 0;
}
