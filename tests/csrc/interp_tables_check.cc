// Host check of tengine_amd/csrc/interp_tables.cc without Python and without a GPU: linked with that file ALONE and built with
// -fsanitize=address,undefined (tests/test_interp_cpu.py).  The command line holds requests, one line of output each:
//   t dtype in_scale in_zp out_scale out_zp      the byte map, 512 hex digits
//   i in_extent out_extent scale                 the index vector, comma separated ("refused" when tamd_interp_indices says -1)
// (scales as the hex bit patterns of the floats).  Then the degenerate inputs: zero scales, empty extents, null pointers, a scale that
// sends an index out of the input -- none may trap, write outside its array (the arrays below are exactly as long as documented, so
// the address sanitizer sees an overrun) or answer 0 where the header says -1.  Exit 0: nothing was flagged.
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
        if (!strcmp(argv[i], "t") && i + 5 < argc) {
            std::vector<unsigned char> table(256);
            if (tamd_interp_table(atoi(argv[i + 1]), bits(argv[i + 2]), atoi(argv[i + 3]), bits(argv[i + 4]), atoi(argv[i + 5]), table.data())) { fprintf(stderr, "request %d: no table\n", i); return 1; }
            for (int b = 0; b < 256; b++) printf("%02x", table[b]);
            printf("\n");
            i += 6;
        } else if (!strcmp(argv[i], "i") && i + 3 < argc) {
            const int out = atoi(argv[i + 2]);
            std::vector<int> idx((size_t)(out > 0 ? out : 0));
            if (tamd_interp_indices(atoi(argv[i + 1]), out, bits(argv[i + 3]), idx.data())) printf("refused\n");
            else {
                for (int o = 0; o < out; o++) printf(o ? ",%d" : "%d", idx[o]);
                printf("\n");
            }
            i += 4;
        } else {
            fprintf(stderr, "usage: t dtype in_scale in_zp out_scale out_zp | i in_extent out_extent scale ...\n");
            return 2;
        }
    }
    std::vector<unsigned char> table(256);
    // a zero scale divides by zero in float (inf / NaN -> INT_MIN, as the reference's x86 code converts it): a table still comes out
    for (int dt : {TAMD_DT_INT8, TAMD_DT_UINT8})
        if (tamd_interp_table(dt, 0.05f, 0, 0.f, 0, table.data()) || tamd_interp_table(dt, 0.f, 0, 0.f, 3, table.data()) || tamd_interp_table(dt, 0.f, 7, 0.02f, 0, table.data())) return 1;
    if (tamd_interp_table(TAMD_DT_FP32, 0.05f, 0, 0.02f, 0, table.data()) != -1 || tamd_interp_table(TAMD_DT_INT32, 0.05f, 0, 0.02f, 0, table.data()) != -1) return 1;
    if (tamd_interp_table(TAMD_DT_UINT8, 0.05f, 0, 0.02f, 0, nullptr) != -1) return 1;
    std::vector<int> four(4), none;
    if (tamd_interp_indices(4, 4, 0.f, four.data()) != -1) return 1;             // 0 / 0 and o / 0: NaN and inf
    if (tamd_interp_indices(4, 4, -1.f, four.data()) != -1) return 1;            // negative source rows
    if (tamd_interp_indices(4, 4, 0.5f, four.data()) != -1) return 1;            // rows 0 2 4 6: 4 leaves the input
    if (tamd_interp_indices(4, 4, 1e-30f, four.data()) != -1) return 1;          // far beyond int
    if (tamd_interp_indices(4, 0, 1.f, none.data()) != -1 || tamd_interp_indices(0, 4, 1.f, four.data()) != -1 || tamd_interp_indices(4, -3, 1.f, none.data()) != -1) return 1;
    if (tamd_interp_indices(4, 4, 1.f, nullptr) != -1) return 1;
    if (tamd_interp_indices(4, 4, 1.f, four.data()) || four[0] != 0 || four[3] != 3) return 1;
    return 0;
}
