// CPU statement of the random numbers gi_sample_rays* and gi_radiance* draw (gi_math.h mx_key, mx_u01k, mx_disk),
// for tests/radiance_ref.py's numpy ports to be compared with, bit for bit.  Reads records from the file argv[1],
// one per line, every number a 64-bit pattern in hex:
//   k <seed> <stream>                      -> mx_key
//   u <key> <sample> <bounce> <dim>        -> the bits of mx_u01k
//   d <bits of u1> <bits of u2>            -> the bits of mx_disk's dx, dy, r2
// and prints one line of hex patterns per record.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "gi_math.h"

static double as_f64(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
static uint64_t as_bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char c;
    uint64_t a[4];
    while (fscanf(f, " %c", &c) == 1) {
        const int want = c == 'k' ? 2 : c == 'u' ? 4 : c == 'd' ? 2 : -1;
        if (want < 0) return 3;
        for (int i = 0; i < want; ++i)
            if (fscanf(f, "%" SCNx64, &a[i]) != 1) return 3;
        if (c == 'k') {
            printf("%016" PRIx64 "\n", gi::mx_key(a[0], a[1]));
        } else if (c == 'u') {
            printf("%016" PRIx64 "\n", as_bits(gi::mx_u01k(a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3])));
        } else {
            double dx, dy, r2;
            gi::mx_disk(as_f64(a[0]), as_f64(a[1]), dx, dy, r2);
            printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", as_bits(dx), as_bits(dy), as_bits(r2));
        }
    }
    fclose(f);
    return 0;
}
