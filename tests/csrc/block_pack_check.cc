// Known-answer test of block_pack.h (the weight blob of block_i8.hip): unpacking each panel by the documented layout
//   [32-row tile][32-deep K step][lane = half * 32 + row][16 B],  lane bytes = k 32 step + 16 half + 0 .. 15
// gives back the OIHW weights, every padding byte is zero, and the three panels sit back to back.  Host compiler only.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "block_pack.h"

using namespace tamd;

// W[row][k] of a panel with `rows` x `K` (both padded) read by walking the layout, not by calling block_panel_at
static std::vector<int8_t> unpack(const int8_t* p, int rows, int K)
{
    std::vector<int8_t> w((size_t)rows * K);
    size_t at = 0;
    for (int tile = 0; tile < rows / 32; tile++)
        for (int step = 0; step < K / 32; step++)
            for (int lane = 0; lane < 64; lane++)
                for (int b = 0; b < 16; b++) w[(size_t)(tile * 32 + lane % 32) * K + step * 32 + (lane / 32) * 16 + b] = p[at++];
    return w;
}

static long check(int C, int mid)
{
    const int mp = block_mid_pad(mid);
    std::vector<int8_t> wa((size_t)mid * C), wb((size_t)mid * mid * 9), wc((size_t)C * mid);
    unsigned s = 12345u + C * 131u + mid;
    auto next = [&]() { s = s * 1664525u + 1013904223u; int v = (int)((s >> 16) % 255) - 127; return (int8_t)(v == 0 ? 1 : v); };    // never 0: padding stands out
    for (auto& v : wa) v = next();
    for (auto& v : wb) v = next();
    for (auto& v : wc) v = next();
    std::vector<int8_t> out(block_packed_bytes(C, mp) + 64, 77);
    block_pack(wa.data(), wb.data(), wc.data(), C, mid, out.data());
    long bad = 0;
    for (size_t i = block_packed_bytes(C, mp); i < out.size(); i++) bad += out[i] != 77;                 // nothing written past the blob
    if (block_packed_bytes(C, mp) != (size_t)2 * mp * C + (size_t)9 * mp * mp) bad++;
    const std::vector<int8_t> ua = unpack(out.data(), mp, C);
    const std::vector<int8_t> ub = unpack(out.data() + (size_t)mp * C, mp, 9 * mp);
    const std::vector<int8_t> uc = unpack(out.data() + (size_t)mp * C + (size_t)9 * mp * mp, C, mp);
    for (int co = 0; co < mp; co++)
        for (int ci = 0; ci < C; ci++) bad += ua[(size_t)co * C + ci] != (co < mid ? wa[(size_t)co * C + ci] : 0);
    for (int co = 0; co < mp; co++)
        for (int tap = 0; tap < 9; tap++)
            for (int ci = 0; ci < mp; ci++)
                bad += ub[(size_t)co * 9 * mp + tap * mp + ci] != (co < mid && ci < mid ? wb[((size_t)co * mid + ci) * 9 + tap] : 0);
    for (int co = 0; co < C; co++)
        for (int ci = 0; ci < mp; ci++) bad += uc[(size_t)co * mp + ci] != (ci < mid ? wc[(size_t)co * mid + ci] : 0);
    return bad;
}

int main()
{
    long bad = 0;
    const int cases[][2] = {{256, 64}, {64, 16}, {128, 32}, {96, 48}, {32, 1}, {64, 33}};
    for (auto& c : cases) bad += check(c[0], c[1]);
    printf("mismatches %ld\n", bad);
    return bad != 0;
}
