// Host check of tengine_amd/csrc/chanmap_tables.cc without Python and without a GPU: linked with that file ALONE and built with
// -fsanitize=address,undefined (tests/test_shuffle_cpu.py).  The command line holds requests, one line of output each:
//   t in_scale in_zp out_scale out_zp      the uint8 Split byte map, 512 hex digits
//   s channels group                       the ShuffleChannel source vector, comma separated ("refused" when the builder says -1)
// (scales as the hex bit patterns of the floats).  Then the degenerate inputs: zero scales, group counts that do not divide, empty
// tensors, null pointers -- none may trap, write outside its array (the arrays below are exactly as long as documented, so the address
// sanitizer sees an overrun) or answer 0 where the header says -1.  Exit 0: nothing was flagged.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/tengine_amd.h"

static float bits(const char* s)
{
    const unsigned u = (unsigned)strtoul(s, nullptr, 16);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main(int argc, char** argv)
{
    for (int i = 1; i < argc;) {
        if (!strcmp(argv[i], "t") && i + 4 < argc) {
            std::vector<unsigned char> table(256);
            if (tamd_split_table(bits(argv[i + 1]), atoi(argv[i + 2]), bits(argv[i + 3]), atoi(argv[i + 4]), table.data())) { fprintf(stderr, "request %d: no table\n", i); return 1; }
            for (int b = 0; b < 256; b++) printf("%02x", table[b]);
            printf("\n");
            i += 5;
        } else if (!strcmp(argv[i], "s") && i + 2 < argc) {
            const int c = atoi(argv[i + 1]);
            std::vector<int> src((size_t)(c > 0 ? c : 0));
            if (tamd_shuffle_sources(c, atoi(argv[i + 2]), src.data())) printf("refused\n");
            else {
                for (int o = 0; o < c; o++) printf(o ? ",%d" : "%d", src[o]);
                printf("\n");
            }
            i += 3;
        } else {
            fprintf(stderr, "usage: t in_scale in_zp out_scale out_zp | s channels group ...\n");
            return 2;
        }
    }
    std::vector<unsigned char> table(256);
    // a zero scale divides by zero in float (inf / NaN -> INT_MIN, as the reference's x86 code converts it): a table still comes out
    if (tamd_split_table(0.05f, 0, 0.f, 0, table.data()) || tamd_split_table(0.f, 0, 0.f, 3, table.data()) || tamd_split_table(0.f, 7, 0.02f, 0, table.data())) return 1;
    if (tamd_split_table(1e30f, 0, 1e-30f, 255, table.data()) || tamd_split_table(-0.05f, 300, 0.02f, -300, table.data())) return 1;
    if (tamd_split_table(0.05f, 0, 0.02f, 0, nullptr) != -1) return 1;
    std::vector<int> twelve(12), none;
    if (tamd_shuffle_sources(12, 5, twelve.data()) != -1 || tamd_shuffle_sources(12, 0, twelve.data()) != -1 || tamd_shuffle_sources(12, -3, twelve.data()) != -1) return 1;
    if (tamd_shuffle_sources(12, 24, twelve.data()) != -1) return 1;              // more groups than channels
    if (tamd_shuffle_sources(0, 1, none.data()) != -1 || tamd_shuffle_sources(-4, 2, none.data()) != -1) return 1;
    if (tamd_shuffle_sources(12, 3, nullptr) != -1) return 1;
    if (tamd_shuffle_sources(12, 3, twelve.data()) || twelve[0] != 0 || twelve[1] != 4 || twelve[2] != 8 || twelve[3] != 1 || twelve[11] != 11) return 1;
    if (tamd_shuffle_sources(12, 12, twelve.data()) || twelve[5] != 5 || tamd_shuffle_sources(12, 1, twelve.data()) || twelve[7] != 7) return 1;
    return 0;
}
