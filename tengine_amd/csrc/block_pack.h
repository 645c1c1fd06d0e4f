// Weight layout of the fused identity-bottleneck kernel (block_i8.hip): the three convolutions' int8 weights as ONE blob in MFMA
// A-fragment order, copied into LDS as it is.  Host code only, no HIP: tests/csrc/block_pack_check.cc compiles it with the host compiler.
//
// A panel is a matrix W[rows][K] cut into 32-row tiles and 32-deep K steps: [tile][K step][lane = half * 32 + row][16 B], the lane's
// bytes being k = 32 step + 16 half + 0 .. 15 of its row (the A operand of v_mfma_i32_32x32x32_i8); rows and K zero padded.
// With mp = mid rounded up to 32:
//   panel a  branch2a 1x1   rows = mp,   K = cin         W[co][ci]                    from OIHW [mid][cin][1][1]
//   panel b  branch2b 3x3   rows = mp,   K = 9 mp        W[co][tap * mp + ci]         from OIHW [mid][mid][3][3], tap = 3 ky + kx
//   panel c  branch2c 1x1   rows = cout, K = mp          W[co][ci]                    from OIHW [cout][mid][1][1]
// cin == cout == C, a multiple of 32.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tamd {

constexpr int block_mid_pad(int mid) { return (mid + 31) / 32 * 32; }
constexpr size_t block_panel_a_bytes(int C, int mp) { return (size_t)mp * C; }
constexpr size_t block_panel_b_bytes(int mp) { return (size_t)9 * mp * mp; }
constexpr size_t block_packed_bytes(int C, int mp) { return 2 * block_panel_a_bytes(C, mp) + block_panel_b_bytes(mp); }

// byte offset of W[row][k] inside a panel of K (a multiple of 32) columns
constexpr size_t block_panel_at(int row, int k, int K)
{
    return (((size_t)(row >> 5) * (K >> 5) + (k >> 5)) * 64 + ((k >> 4) & 1) * 32 + (row & 31)) * 16 + (k & 15);
}

// wa / wb / wc: the three nodes' weights in the model's OIHW order; out: block_packed_bytes(C, block_mid_pad(mid)) bytes
inline void block_pack(const int8_t* wa, const int8_t* wb, const int8_t* wc, int C, int mid, int8_t* out)
{
    const int mp = block_mid_pad(mid);
    for (size_t i = 0; i < block_packed_bytes(C, mp); i++) out[i] = 0;
    int8_t* pa = out;
    int8_t* pb = pa + block_panel_a_bytes(C, mp);
    int8_t* pc = pb + block_panel_b_bytes(mp);
    for (int co = 0; co < mid; co++)
        for (int ci = 0; ci < C; ci++) pa[block_panel_at(co, ci, C)] = wa[(size_t)co * C + ci];
    for (int co = 0; co < mid; co++)
        for (int ci = 0; ci < mid; ci++)
            for (int tap = 0; tap < 9; tap++) pb[block_panel_at(co, tap * mp + ci, 9 * mp)] = wb[((size_t)co * mid + ci) * 9 + tap];
    for (int co = 0; co < C; co++)
        for (int ci = 0; ci < mid; ci++) pc[block_panel_at(co, ci, mp)] = wc[(size_t)co * mid + ci];
}

}  // namespace tamd
