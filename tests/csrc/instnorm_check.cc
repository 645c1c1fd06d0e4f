// tamd_instancenorm_plane and instancenorm_bound (csrc/instnorm_tables.cc / .h) as a stand-alone host program: tests/test_instnorm_cpu.py
// builds this file and instnorm_tables.cc, nothing else, with -fsanitize=address,undefined and compares every line with what the library
// answers for the same plane.
// stdin, one plane per line:  size lo hi seed gamma beta eps in_scale in_zp out_scale out_zp
//   the plane holds `size` bytes drawn from lo .. hi by the generator below (size 0: a null plane, which the function refuses)
// stdout, one line per plane: rc sum sqsum a b (the four as hex bit patterns) fnv1a(table) bound
// The plane lies in a heap block of exactly `size` bytes, so a read past either end is the sanitizer's.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "instnorm_tables.h"

static unsigned bits(float f)
{
    unsigned u;
    memcpy(&u, &f, 4);
    return u;
}

int main()
{
    int size, lo, hi, in_zp, out_zp;
    unsigned seed;
    float gamma, beta, eps, in_scale, out_scale;
    while (scanf("%d %d %d %u %f %f %f %f %d %f %d", &size, &lo, &hi, &seed, &gamma, &beta, &eps, &in_scale, &in_zp, &out_scale, &out_zp) == 11) {
        std::vector<unsigned char> x((size_t)(size > 0 ? size : 0));
        unsigned s = seed * 2654435761u + 12345u;
        for (int j = 0; j < size; j++) {
            s = s * 1664525u + 1013904223u;
            x[(size_t)j] = (unsigned char)(lo + (int)((s >> 8) % (unsigned)(hi - lo + 1)));
        }
        unsigned char table[256];
        float st[4] = {0.f, 0.f, 0.f, 0.f};
        memset(table, 0, sizeof(table));
        const int rc = tamd_instancenorm_plane(size > 0 ? x.data() : nullptr, size, gamma, beta, eps, in_scale, in_zp, out_scale, out_zp, table, st);
        unsigned h = 2166136261u;
        for (int b = 0; b < 256; b++) h = (h ^ table[b]) * 16777619u;
        const double bound = tamd::instancenorm_bound(&gamma, &beta, 1, eps, in_scale, out_scale, out_zp);
        printf("%d %08x %08x %08x %08x %08x %.6e\n", rc, bits(st[0]), bits(st[1]), bits(st[2]), bits(st[3]), h, bound);
    }
    return 0;
}
