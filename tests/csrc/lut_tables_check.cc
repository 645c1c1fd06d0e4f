// Host check of tengine_amd/csrc/lut_tables.cc without Python and without a GPU: linked with that file ALONE and built with
// -fsanitize=address,undefined (tests/test_lut_cpu.py), it builds the table of every parameter set given on the command line --
// groups of eight values: op dtype in_scale in_zp out_scale out_zp p0 p1 (scales and p0 / p1 as the hex bit patterns of the floats)
// -- prints each as 512 hex digits, then asks for every (op, dtype) pair the header knows and checks that exactly the six documented
// ones answer.  Exit 0: every table was built and nothing was flagged.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
    if ((argc - 1) % 8) { fprintf(stderr, "usage: groups of op dtype in_scale in_zp out_scale out_zp p0 p1\n"); return 2; }
    for (int i = 1; i + 7 < argc; i += 8) {
        const float p[2] = {bits(argv[i + 6]), bits(argv[i + 7])};
        unsigned char table[256];
        if (tamd_lut_table(atoi(argv[i]), atoi(argv[i + 1]), p, bits(argv[i + 2]), atoi(argv[i + 3]), bits(argv[i + 4]), atoi(argv[i + 5]), table)) {
            fprintf(stderr, "set %d: no table\n", (i - 1) / 8);
            return 1;
        }
        for (int b = 0; b < 256; b++) printf("%02x", table[b]);
        printf("\n");
    }
    int answered = 0;
    unsigned char table[256];
    const float p[2] = {6.f, 0.f};
    for (int op = 0; op < TAMD_OP_NUM; op++)
        for (int dt = TAMD_DT_FP32; dt <= TAMD_DT_INT32; dt++)
            if (tamd_lut_table(op, dt, p, 0.05f, 0, 0.02f, 0, table) == 0) {
                const bool both = op == TAMD_OP_SIGMOID || op == TAMD_OP_CLIP, u8_only = op == TAMD_OP_HARDSWISH || op == TAMD_OP_MISH;
                if (!((both && (dt == TAMD_DT_INT8 || dt == TAMD_DT_UINT8)) || (u8_only && dt == TAMD_DT_UINT8))) { fprintf(stderr, "unexpected table for op %d dtype %d\n", op, dt); return 1; }
                answered++;
            }
    if (answered != 6) { fprintf(stderr, "%d pairs answered, 6 expected\n", answered); return 1; }
    // degenerate quantisation parameters must not trap either: a zero scale divides by zero in float (inf / NaN -> INT_MIN, as the reference's x86 code converts it)
    for (int op = TAMD_OP_SIGMOID; op <= TAMD_OP_MISH; op++)
        if (tamd_lut_table(op, TAMD_DT_UINT8, p, 0.05f, 0, 0.f, 0, table) || tamd_lut_table(op, TAMD_DT_UINT8, p, 0.f, 0, 0.f, 3, table)) return 1;
    if (tamd_lut_table(TAMD_OP_CLIP, TAMD_DT_UINT8, nullptr, 0.05f, 0, 0.02f, 0, table) != -1) return 1;      // Clip without its parameters
    return 0;
}
