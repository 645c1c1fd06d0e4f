// Phase anatomy of the fused identity-bottleneck kernel (block_i8.hip) on the 100 MHz wall clock: the product source compiled with
// TAMD_BLOCK_STAMPS on ResNet-50's res2b / res2c shape (56x56, 256 -> 64 -> 64 -> 256) at batch 32, random operands (timing only; the
// requantisation constants are plausible, not a model's).  Wave 0 of every block adds up, over its tiles, the time between the stamps:
//   prologue (weights + constants + first tile -> LDS) | phase A (branch2a on tile + halo) | phase B (3x3) | phase C (branch2c + residual
//   + stores issued) | next tile's input registers -> LDS
// Printed: us per launch (events, 20 dependent launches), then the mean over the blocks of each sum and of the whole block, us.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -mllvm --amdgpu-mfma-vgpr-form -DTAMD_BLOCK_STAMPS -I../../tengine_amd/csrc -o block_anatomy.bin block_anatomy.hip
#include "../../tengine_amd/csrc/block_i8.hip"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); exit(1); } } while (0)

namespace tamd {
thread_local std::vector<LaunchRec>* g_launch_rec = nullptr;
thread_local bool g_launch_coherent = false;
thread_local bool g_launch_beside = false;
}
using namespace tamd;

int main(int argc, char** argv)
{
    const int N = argc > 1 ? atoi(argv[1]) : 32, HW = argc > 2 ? atoi(argv[2]) : 56, C = argc > 3 ? atoi(argv[3]) : 256, MID = argc > 4 ? atoi(argv[4]) : 64;
    const int L = 20, reps = 10;
    if (C % 32 != 0 || C > 256 || MID > 64) { fprintf(stderr, "shape outside block_applicable\n"); return 1; }
    hipStream_t st;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    const size_t tens = (size_t)N * HW * HW * C + 65536;
    const int mp = block_mid_pad(MID);
    int8_t *x, *y, *wpk; int* bias; float* scale; unsigned long long* stamps;
    CK(hipMalloc(&x, tens)); CK(hipMalloc(&y, tens)); CK(hipMalloc(&wpk, block_packed_bytes(C, mp))); CK(hipMalloc(&bias, 1 << 12)); CK(hipMalloc(&scale, 1 << 12));
    std::vector<int8_t> r(tens);
    unsigned s = 12345u;
    for (auto& v : r) { s = s * 1664525u + 1013904223u; v = (int8_t)(s >> 24); }
    CK(hipMemcpy(x, r.data(), tens, hipMemcpyHostToDevice));
    CK(hipMemcpy(wpk, r.data() + 4096, block_packed_bytes(C, mp), hipMemcpyHostToDevice));
    CK(hipMemset(bias, 0, 1 << 12));
    std::vector<float> sc(1 << 10, 0.0005f);
    CK(hipMemcpy(scale, sc.data(), 1 << 12, hipMemcpyHostToDevice));

    ConvArgs a{}, b{}, c{};
    a.x = x; a.N = N; a.H = a.OH = HW; a.W = a.OW = HW; a.cs_in = C; a.cin = C; a.cout = MID; a.KH = a.KW = a.SH = a.SW = a.DH = a.DW = 1;
    a.bias = bias; a.wscale = scale; a.rq = {0.05f, 0.f, 12.f, 0.1f, 128.25f, 248.75f, 0x1p-13f, scale};
    b = a; b.cin = MID; b.KH = b.KW = 3; b.PH = b.PW = 1;
    c = a; c.cin = MID; c.cout = C; c.y = y; c.ldc = C; c.c_off = 0; c.c_limit = C;
    c.rq = {0.05f, -12.f, 12.f, 0.1f, 8.25f, 248.75f, 0x1p-13f, scale};
    c.elt.res = x; c.elt.res_ldc = C; c.elt.res_c_off = 0; c.elt.type = 2; c.elt.s_conv = 0.1f; c.elt.s_res = 0.08f; c.elt.out_scale = 0.15f;
    c.elt.relu = 2; c.elt.relu_out_scale = 0.15f;
    const float eps = 0x1p-13f;
    c.elt.mc = 0.1f / 0.15f; c.elt.mr = 0.08f / 0.15f; c.elt.k0 = 128.5f + eps - 128.f * (c.elt.mc + c.elt.mr); c.elt.ylo = 128.25f; c.elt.yhi = 255.75f; c.elt.thr = 2.f * eps;
    if (!block_applicable(a, b, c)) { fprintf(stderr, "block_applicable says no\n"); return 1; }
    BlockArgs v = block_args(a, b, c, wpk);
    CK(hipMalloc(&stamps, (size_t)v.grid * 8 * 8));
    CK(hipMemset(stamps, 0, (size_t)v.grid * 8 * 8));
    v.stamps = stamps;
    printf("block_i8 %dx%dx%d, mid %d, batch %d: %d tiles on %d blocks of %d threads, %zu B of LDS\n", HW, HW, C, MID, N, v.tiles, v.grid, BLK_THREADS, block_lds_bytes(C, mp));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 3; i++) CK(launch_block(v, st));
    CK(hipStreamSynchronize(st));
    float best = 1e9f;
    for (int rep = 0; rep < reps; rep++) {
        CK(hipEventRecord(e0, st));
        for (int i = 0; i < L; i++) CK(launch_block(v, st));
        CK(hipEventRecord(e1, st));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best) best = ms;
    }
    std::vector<unsigned long long> h((size_t)v.grid * 8);
    CK(hipMemcpy(h.data(), stamps, h.size() * 8, hipMemcpyDeviceToHost));
    double sum[5] = {0, 0, 0, 0, 0}, all = 0;
    for (int bl = 0; bl < v.grid; bl++)
        for (int i = 0; i < 5; i++) { sum[i] += h[(size_t)bl * 8 + i] / 100.0; all += h[(size_t)bl * 8 + i] / 100.0; }
    printf("us per launch (fastest of %d x %d dependent launches): %.2f\n", reps, L, 1e3 * best / L);
    printf("per block, mean over %d blocks (%.2f tiles each), us: prologue %.2f | phase A %.2f | phase B %.2f | phase C %.2f | next input -> LDS %.2f | whole block %.2f\n",
           v.grid, (double)v.tiles / v.grid, sum[0] / v.grid, sum[1] / v.grid, sum[2] / v.grid, sum[3] / v.grid, sum[4] / v.grid, all / v.grid);
    return 0;
}
