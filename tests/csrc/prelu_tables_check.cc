// Host check of tengine_amd/csrc/prelu_tables.cc without Python and without a GPU: linked with that file ALONE and built with
// -fsanitize=address,undefined (tests/test_prelu_cpu.py).  It builds the table of every parameter set given on the command line --
// groups of six values: dtype slope_bits in_scale in_zp out_scale out_zp (slope_bits and the scales as hex bit patterns) -- and prints
// each as 512 hex digits; then it widens all 65 536 halves and prints how many differ from the IEEE widening, builds tables with
// degenerate quantisation parameters (scale 0, a denormal scale, zero point 255) for every slope pattern of interest, and checks what
// must be refused.  Exit 0: every table was built and nothing was flagged.
#include <math.h>
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

static unsigned pattern(float f)
{
    unsigned u;
    memcpy(&u, &f, 4);
    return u;
}

// IEEE binary16 -> binary32, for the count alone
static unsigned ieee_widen(unsigned h)
{
    const unsigned sign = (h >> 15) << 31, exp = (h >> 10) & 0x1f;
    unsigned frac = h & 0x3ff;
    if (exp == 31) return sign | 0xffu << 23 | frac << 13;
    if (exp) return sign | (exp + 112) << 23 | frac << 13;
    if (!frac) return sign;
    int e = 113;
    while (!(frac & 0x400)) { frac <<= 1; e--; }
    return sign | (unsigned)e << 23 | (frac & 0x3ff) << 13;
}

int main(int argc, char** argv)
{
    if ((argc - 1) % 6) { fprintf(stderr, "usage: groups of dtype slope_bits in_scale in_zp out_scale out_zp\n"); return 2; }
    unsigned char table[256];
    for (int i = 1; i + 5 < argc; i += 6) {
        if (tamd_prelu_table(atoi(argv[i]), (unsigned short)strtoul(argv[i + 1], nullptr, 16), bits(argv[i + 2]), atoi(argv[i + 3]), bits(argv[i + 4]), atoi(argv[i + 5]), table)) {
            fprintf(stderr, "set %d: no table\n", (i - 1) / 6);
            return 1;
        }
        for (int b = 0; b < 256; b++) printf("%02x", table[b]);
        printf("\n");
    }
    // the widening: every pattern; the quirks by name
    int differ = 0, nonfinite = 0;
    for (unsigned h = 0; h < 65536; h++) {
        const float f = tamd_prelu_slope((unsigned short)h);
        if (!isfinite(f)) nonfinite++;
        if (pattern(f) != ieee_widen(h)) differ++;
    }
    // 60 normal powers of two, 2026 sub-normals (the 20 sub-normal powers of two come out right), 2046 NaNs; 2046 NaNs + 2 infinities
    printf("differ %d nonfinite %d\n", differ, nonfinite);
    if (differ != 4132 || nonfinite != 2048) { fprintf(stderr, "the widening's quirks changed\n"); return 1; }
    if (pattern(tamd_prelu_slope(0x3400)) != 0u || pattern(tamd_prelu_slope(0xbc00)) != 0u) { fprintf(stderr, "a power of two must widen to +0\n"); return 1; }
    if (pattern(tamd_prelu_slope(0x0003)) != 0x34000200u || pattern(tamd_prelu_slope(0x8000)) != 0x80000000u) { fprintf(stderr, "sub-normal / -0\n"); return 1; }
    if (pattern(tamd_prelu_slope(0x7c00)) != 0x7f800000u || pattern(tamd_prelu_slope(0xfe00)) != 0xff800001u) { fprintf(stderr, "inf / NaN\n"); return 1; }
    // degenerate quantisation parameters must not trap: a zero scale divides by zero in float (inf / NaN -> INT_MIN, as the reference's
    // x86 code converts it), a denormal one overflows the quotient
    const unsigned short slopes[] = {0x3400, 0x0000, 0x2e66, 0xb4cd, 0x4400, 0x429a, 0x0003, 0x8000, 0x03ff, 0x7bff, 0xfbff};
    const float denormal = bits("00000001");
    for (unsigned short s : slopes)
        for (int dt = TAMD_DT_INT8; dt <= TAMD_DT_UINT8; dt++) {
            const int zp = dt == TAMD_DT_UINT8 ? 255 : 0;
            if (tamd_prelu_table(dt, s, 0.05f, zp, 0.f, zp, table) || tamd_prelu_table(dt, s, 0.f, 0, 0.f, 3, table) || tamd_prelu_table(dt, s, denormal, zp, denormal, 0, table)
                || tamd_prelu_table(dt, s, 0.05f, 0, denormal, zp, table) || tamd_prelu_table(dt, s, 3e38f, zp, 0.02f, 0, table))
                return 1;
        }
    // int8 never gives -128, whatever goes in
    if (tamd_prelu_table(TAMD_DT_INT8, 0x429a, 0.05f, 0, 0.001f, 0, table)) return 1;
    for (int b = 0; b < 256; b++)
        if (table[b] == 0x80) { fprintf(stderr, "-128 came out\n"); return 1; }
    if (table[0x80] != 0x81 || table[0x7f] != 0x7f) { fprintf(stderr, "the ends do not saturate\n"); return 1; }
    // refused: other types, non-finite slopes, no table
    const int other_types[] = {TAMD_DT_FP32, TAMD_DT_FP16, TAMD_DT_INT32, 7};
    for (int dt : other_types)
        if (tamd_prelu_table(dt, 0x2e66, 0.05f, 0, 0.02f, 0, table) != -1) return 1;
    const unsigned short nonfinite_slopes[] = {0x7c00, 0xfc00, 0x7e00, 0x7c01};
    for (unsigned short s : nonfinite_slopes)
        if (tamd_prelu_table(TAMD_DT_INT8, s, 0.05f, 0, 0.02f, 0, table) != -1 || tamd_prelu_table(TAMD_DT_UINT8, s, 0.05f, 0, 0.02f, 0, table) != -1) return 1;
    if (tamd_prelu_table(TAMD_DT_INT8, 0x2e66, 0.05f, 0, 0.02f, 0, nullptr) != -1) return 1;
    return 0;
}
