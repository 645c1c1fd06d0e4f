// Host check of the Eltwise byte maps of tengine_amd/csrc/lut_tables.cc without Python and without a GPU: linked with that file ALONE
// and built with -fsanitize=address,undefined (tests/test_bytemap_cpu.py), it builds the table of every parameter set given on the
// command line -- groups of ten values: type dtype in_scale in_zp out_scale out_zp scalar shift power scale (the floats as hex bit
// patterns) -- and prints each as 512 hex digits, then a checksum line over all 65 536 byte pairs of PROD / SUM / SUB / MAX in both
// types, then walks what must be refused: every type without a case (-1), tables with an undefined entry (-2: NaN, infinity, outside
// int -- the float-to-int conversions the sanitizer would flag are exactly the ones the builder must not reach), degenerate scales.
// Exit 0: every table was built and nothing was flagged.
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

int main(int argc, char** argv)
{
    if ((argc - 1) % 10) { fprintf(stderr, "usage: groups of type dtype in_scale in_zp out_scale out_zp scalar shift power scale\n"); return 2; }
    unsigned char table[256];
    for (int i = 1; i + 9 < argc; i += 10) {
        const int type = atoi(argv[i]);
        const tamd_eltwise_param p = {type, 1, bits(argv[i + 7]), bits(argv[i + 8]), bits(argv[i + 9])};
        const int rc = tamd_eltwise_table(type, atoi(argv[i + 1]), &p, bits(argv[i + 6]), bits(argv[i + 2]), atoi(argv[i + 3]), bits(argv[i + 4]), atoi(argv[i + 5]), table);
        if (rc) { fprintf(stderr, "set %d: no table (%d)\n", (i - 1) / 10, rc); return 1; }
        for (int b = 0; b < 256; b++) printf("%02x", table[b]);
        printf("\n");
    }
    // every byte pair of the same-shape forms: a checksum the test compares with the library's
    for (int dt = TAMD_DT_INT8; dt <= TAMD_DT_UINT8; dt++)
        for (int type = 0; type <= 6; type += 2) {
            unsigned long sum = 0;
            for (int a = 0; a < 256; a++)
                for (int b = 0; b < 256; b++) {
                    const int v = tamd_eltwise_pair(type, dt, (unsigned char)a, 0.05f, dt == TAMD_DT_UINT8 ? 100 : 0, (unsigned char)b, 0.02f, dt == TAMD_DT_UINT8 ? 140 : 0, 0.05f,
                                                    dt == TAMD_DT_UINT8 ? 128 : 0);
                    if (v < 0 || v > 255) { fprintf(stderr, "pair %d %d %d %d: %d\n", dt, type, a, b, v); return 1; }
                    sum = sum * 31 + (unsigned long)v;
                }
            printf("pairs %d %d %lu\n", dt, type, sum);
        }
    // what has no table
    const tamd_eltwise_param p = {17, 1, 0.f, 2.f, 1.f};
    for (int type = -1; type <= 20; type++) {
        const bool has = type == 0 || type == 1 || type == 2 || type == 4 || type == 5 || type == 7 || type == 8 || (type >= 10 && type <= 15) || type == 17;
        for (int dt = TAMD_DT_FP32; dt <= TAMD_DT_INT32; dt++) {
            // (uint8 zero point -1, scalar 0.5: x > 0 on every byte, so every type with a case is defined; int8 reaches x < 0: RSQRT, LOG and SQRT are not)
            const int rc = tamd_eltwise_table(type, dt, &p, 0.5f, 0.05f, dt == TAMD_DT_UINT8 ? -1 : 0, 0.05f, 0, table);
            const bool quantised = dt == TAMD_DT_INT8 || dt == TAMD_DT_UINT8;
            const bool nan_i8 = dt == TAMD_DT_INT8 && (type == 7 || type == 11 || type == 13);
            const int want = !has || !quantised ? -1 : nan_i8 ? -2 : 0;
            if (rc != want) { fprintf(stderr, "type %d dtype %d: %d, %d expected\n", type, dt, rc, want); return 1; }
        }
    }
    if (tamd_eltwise_table(17, TAMD_DT_UINT8, nullptr, 0.f, 0.05f, 0, 0.05f, 0, table) != -1) return 1;                // POWER without its parameters
    if (tamd_eltwise_table(0, TAMD_DT_UINT8, nullptr, 2.f, 0.05f, 0, 0.05f, 0, nullptr) != -1) return 1;
    // undefined entries: 1 / sqrt(0) and log(0) at the zero-point byte, x / 0, a zero and a NaN output scale, a value outside int, exp overflow
    if (tamd_eltwise_table(7, TAMD_DT_UINT8, &p, 0.f, 0.05f, 0, 0.05f, 0, table) != -2) return 1;
    if (tamd_eltwise_table(11, TAMD_DT_UINT8, &p, 0.f, 0.05f, 0, 0.05f, 0, table) != -2) return 1;
    if (tamd_eltwise_table(10, TAMD_DT_INT8, &p, 0.f, 0.05f, 0, 0.05f, 0, table) != -2) return 1;
    if (tamd_eltwise_table(2, TAMD_DT_UINT8, &p, 1.f, 0.05f, 0, 0.f, 0, table) != -2) return 1;
    if (tamd_eltwise_table(2, TAMD_DT_INT8, &p, 1.f, 0.05f, 0, NAN, 0, table) != -2) return 1;
    if (tamd_eltwise_table(1, TAMD_DT_UINT8, &p, 3.0e38f, 1.f, 0, 1.f, 0, table) != -2) return 1;
    if (tamd_eltwise_table(1, TAMD_DT_UINT8, &p, 1.f, 1.f, 0, 1e-9f, 0, table) != -2) return 1;                       // 255e9: outside int
    if (tamd_eltwise_table(12, TAMD_DT_UINT8, &p, 0.f, 1.f, 0, 1.f, 0, table) != -2) return 1;                        // exp(255)
    if (tamd_eltwise_table(2, TAMD_DT_UINT8, &p, 1.f, 0.05f, 0, 0.05f, 2147483647, table) != -2) return 1;            // round() + zero leaves int
    if (tamd_eltwise_pair(0, TAMD_DT_UINT8, 255, 3.0e38f, 0, 255, 3.0e38f, 0, 1.f, 0) != -2) return 1;
    if (tamd_eltwise_pair(1, TAMD_DT_UINT8, 1, 1.f, 0, 1, 1.f, 0, 1.f, 0) != -1 || tamd_eltwise_pair(0, TAMD_DT_FP32, 1, 1.f, 0, 1, 1.f, 0, 1.f, 0) != -1) return 1;
    // the BatchNorm's per-channel map: mixed signs, a tiny variance, rescale 0 and 1, caffe and not; then what is not finite
    {
        unsigned long sum = 0;
        for (int caffe = 0; caffe < 2; caffe++)
            for (int k = 0; k < 16; k++) {
                const tamd_batchnorm_param bp = {k % 3 ? 1.f : 0.f, k % 2 ? 2e-5f : 1e-3f, caffe};
                const float gamma = (k % 2 ? -1.f : 1.f) * (0.2f + 0.11f * k), beta = 0.4f * (k - 8), mean = 0.1f * (k - 5), var = k % 5 ? 0.3f * k : 1e-7f;
                if (tamd_batchnorm_table(&bp, gamma, beta, mean, var, 0.05f, 128, 0.04f, 120, table)) { fprintf(stderr, "batchnorm %d %d: no table\n", caffe, k); return 1; }
                for (int b = 0; b < 256; b++) sum = sum * 31 + table[b];
            }
        printf("batchnorm %lu\n", sum);
        const tamd_batchnorm_param bp = {1.f, 1e-5f, 0};
        if (tamd_batchnorm_table(nullptr, 1.f, 0.f, 0.f, 1.f, 0.05f, 128, 0.04f, 120, table) != -1 || tamd_batchnorm_table(&bp, 1.f, 0.f, 0.f, 1.f, 0.05f, 128, 0.04f, 120, nullptr) != -1) return 1;
        if (tamd_batchnorm_table(&bp, 1.f, 0.f, 0.f, -1.f, 0.05f, 128, 0.04f, 120, table) != -2) return 1;             // sqrtf of a negative: NaN
        if (tamd_batchnorm_table(&bp, INFINITY, 0.f, 0.f, 1.f, 0.05f, 128, 0.04f, 120, table) != -2) return 1;
        if (tamd_batchnorm_table(&bp, 1.f, 0.f, 0.f, 1.f, 0.05f, 128, 0.f, 120, table) != -2) return 1;                // x / 0
        if (tamd_batchnorm_table(&bp, 3.0e38f, 0.f, 0.f, 1e-30f, 1.f, 0, 1.f, 0, table) != -2) return 1;               // s2 overflows
        if (tamd_batchnorm_table(&bp, 1.f, 0.f, 0.f, 1.f, 1.f, 0, 1e-9f, 0, table) != -2) return 1;                    // 255e9: outside int
    }
    // the constant's value
    float s = 0.f;
    const unsigned char u = 3;
    const signed char q = -128;
    const float f = -1.75f;
    if (tamd_eltwise_scalar(TAMD_DT_UINT8, &u, 0.5f, 5, &s) || s != -1.f) return 1;
    if (tamd_eltwise_scalar(TAMD_DT_INT8, &q, 0.5f, 77, &s) || s != -64.f) return 1;                                  // (an int8 tensor has no zero point)
    if (tamd_eltwise_scalar(TAMD_DT_FP32, &f, 0.f, 0, &s) || s != -1.75f) return 1;
    if (tamd_eltwise_scalar(TAMD_DT_FP16, &f, 0.f, 0, &s) != -1 || tamd_eltwise_scalar(TAMD_DT_FP32, nullptr, 0.f, 0, &s) != -1) return 1;
    return 0;
}
