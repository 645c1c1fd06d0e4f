// Host check of the arithmetic behind the two slots of a graph (tengine_amd/csrc/graph_slots.h: slot_range_of, slot_merge, slot_place,
// slot_rebase): which bytes become private to slot 1 and which kernel-argument words move there.  No device, no HIP.
// build: c++ -std=c++17 -I tengine_amd/csrc slot_rebase_check.cc -o slot_rebase_check
#include <cstdio>

#include "graph_slots.h"

using namespace tamd;

static int bad = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); bad++; } } while (0)

struct Acc { const char* base; size_t size, off, len, period; };          // the fields of tamd::Access (graph.h)

static SlotRange range(uintptr_t lo, size_t bytes) { SlotRange r; r.lo = lo; r.bytes = bytes; return r; }

int main()
{
    const uintptr_t T = 0x7f0000100000ull;            // a tensor: [T, T + 4096)
    const uintptr_t W = 0x7f0000200000ull;            // weights, never written: shared
    const uintptr_t U = 0x7f0000300100ull;            // two wr ranges that touch: [U, U + 512) and [U + 512, U + 1024)
    size_t total = 0;
    std::vector<SlotSpan> sp = slot_merge({range(U + 512, 512), range(T, 4096), range(U, 512), range(0, 64), range(T + 100, 0)}, &total);
    EXPECT(sp.size() == 2);                           // (the null range and the empty one are dropped)
    EXPECT(sp[0].lo == T && sp[0].hi == T + 4096);
    EXPECT(sp[1].lo == U && sp[1].hi == U + 1024);    // two adjacent wr ranges merged into one span
    EXPECT(sp[0].off >= kSlotPad && sp[1].off >= sp[0].off + 4096 + kSlotPad && total >= sp[1].off + 1024 + kSlotPad);
    EXPECT((sp[0].off & 255) == (T & 255) && (sp[1].off & 255) == (U & 255));      // alignment inside a 256-byte granule kept
    const uintptr_t B = 0x7e0000000000ull;            // where slot 1's copy lives
    slot_place(sp, B);
    EXPECT(slot_moved(sp, T) == B + sp[0].off);                                     // a span's first byte
    EXPECT(slot_moved(sp, T + 1234) == B + sp[0].off + 1234);                       // inside
    EXPECT(slot_moved(sp, T + 4095) == B + sp[0].off + 4095);                       // the last byte
    EXPECT(slot_moved(sp, T + 4096) == T + 4096);                                   // one past the end: not moved
    EXPECT(slot_moved(sp, T - 1) == T - 1);                                         // below the start: not moved
    EXPECT(slot_moved(sp, U + 512) == B + sp[1].off + 512);                         // the seam of the merged ranges: one distance
    EXPECT(slot_moved(sp, U + 1024) == U + 1024 && slot_moved(sp, W) == W && slot_moved(sp, 0) == 0);
    EXPECT(slot_touches(sp, T + 4000, 200) && !slot_touches(sp, T + 4096, 64) && !slot_touches(sp, W, 1 << 20) && slot_touches(sp, T - 8, 9));

    // overlapping ranges (tensors of disjoint lifetimes that share pooled memory) are one span too
    std::vector<SlotSpan> ov = slot_merge({range(T, 1000), range(T + 500, 1000), range(T + 200, 100)}, nullptr);
    EXPECT(ov.size() == 1 && ov[0].lo == T && ov[0].hi == T + 1500);

    // a periodic Access (channels [16, 32) of every 64-byte pixel, 100 pixels): the whole [base, base + size) is private
    Acc slice{(const char*)T, 6400, 16, 16, 64};
    SlotRange pr = slot_range_of(slice);
    EXPECT(pr.lo == T && pr.bytes == 6400);
    std::vector<SlotSpan> ps = slot_merge({pr}, nullptr);
    slot_place(ps, B);
    EXPECT(ps.size() == 1 && slot_moved(ps, T) != T && slot_moved(ps, T + 3 * 64 + 40) == slot_moved(ps, T) + 3 * 64 + 40 && slot_moved(ps, T + 6399) != T + 6399);

    // an argument segment: [pointer into T][pointer to weights][two ints][pointer at T's end][pointer below T][pointer into U][4 odd bytes]
    unsigned char seg[8 * 7 + 4];
    const uint64_t words[7] = {T + 64, W + 8, ((uint64_t)7 << 32) | 224u, T + 4096, T - 8, U + 1000, 0};
    memcpy(seg, words, 8 * 6);
    const uint64_t tail_ptr = T + 16;                 // the segment ends 4 bytes into this word: not a whole word, left alone
    memcpy(seg + 48, &tail_ptr, 8);
    const unsigned char odd[4] = {0xde, 0xad, 0xbe, 0xef};
    memcpy(seg + 56, odd, 4);
    unsigned char before[sizeof(seg)];
    memcpy(before, seg, sizeof(seg));
    // 52 bytes: six whole words and four bytes of the seventh
    EXPECT(slot_rebase(seg, 52, sp) == 2);
    uint64_t got[7];
    memcpy(got, seg, 56);
    EXPECT(got[0] == B + sp[0].off + 64);
    EXPECT(got[1] == W + 8);                          // a word inside a shared (weight) range: untouched
    EXPECT(got[2] == words[2] && got[3] == T + 4096 && got[4] == T - 8);
    EXPECT(got[5] == B + sp[1].off + 1000);
    EXPECT(got[6] == tail_ptr && memcmp(seg + 56, odd, 4) == 0);          // the length is no multiple of 8: the tail stays
    EXPECT(memcmp(seg + 8, before + 8, 32) == 0);
    // the whole segment (60 bytes): now the seventh word is a whole word and moves; the last four bytes still stay
    EXPECT(slot_rebase(seg, sizeof(seg), sp) == 1);
    memcpy(got, seg, 56);
    EXPECT(got[6] == B + sp[0].off + 16 && got[0] == B + sp[0].off + 64 && memcmp(seg + 56, odd, 4) == 0);
    // segments shorter than a word, and an empty one
    unsigned char small[7] = {1, 2, 3, 4, 5, 6, 7};
    EXPECT(slot_rebase(small, 7, sp) == 0 && small[0] == 1 && small[6] == 7 && slot_rebase(small, 0, sp) == 0);
    // no spans: nothing moves
    memcpy(seg, before, sizeof(seg));
    EXPECT(slot_rebase(seg, sizeof(seg), std::vector<SlotSpan>()) == 0 && memcmp(seg, before, sizeof(seg)) == 0);

    printf("%d failures\n", bad);
    return bad ? 1 : 0;
}
