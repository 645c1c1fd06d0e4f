// Two slots behind one handle (graph_slots.hip): the arithmetic, host-only -- no HIP in here, so tests/csrc/slot_rebase_check.cc
// runs it on the CPU.
//
// Slot 1 of a graph is a second copy of everything a pass WRITES (tensors, output staging buffers), in one allocation, and the
// recorded launch list with every kernel-argument pointer into those bytes moved to the copy.  What a pass writes is a list of byte
// ranges; overlapping and touching ranges merge into spans; each span has one place in the copy, so every pointer into a span moves
// by that span's constant distance and keeps whatever offset and alignment it had.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace tamd {

struct SlotRange { uintptr_t lo = 0; size_t bytes = 0; };          // [lo, lo + bytes): written by a pass
struct SlotSpan {
    uintptr_t lo = 0, hi = 0;      // [lo, hi) in slot 0's memory
    size_t off = 0;                // where the span begins inside slot 1's allocation
    intptr_t delta = 0;            // slot 1's address of a byte = slot 0's + delta (slot_place)
};

// what an Access (graph.h) makes private.  A periodic Access -- a channel slice of a concat buffer: `len` bytes at `off` of every
// `period` -- makes the WHOLE [base, base + size) private: the other slices of the same pixels are written by other launches of the
// same pass, and a pointer into the buffer must not depend on which slice it serves
template <typename A>
inline SlotRange slot_range_of(const A& a)
{
    SlotRange x;
    x.lo = (uintptr_t)a.base; x.bytes = a.size;
    return x;
}

// room in front of the first span and behind every span: kernels read whole K steps past a buffer's last pixel (dev_alloc keeps 1024
// readable bytes behind every buffer for that); the copy keeps more on both sides
constexpr size_t kSlotPad = 4096;

// ranges -> spans, sorted by address; ranges that overlap or touch become one span.  Every span keeps its address modulo 256 (the
// granule of dev_alloc) in the copy.  *total = bytes the copy needs, padding included
inline std::vector<SlotSpan> slot_merge(std::vector<SlotRange> r, size_t* total)
{
    r.erase(std::remove_if(r.begin(), r.end(), [](const SlotRange& x) { return x.bytes == 0 || x.lo == 0; }), r.end());
    std::sort(r.begin(), r.end(), [](const SlotRange& a, const SlotRange& b) { return a.lo < b.lo; });
    std::vector<SlotSpan> spans;
    for (const SlotRange& x : r) {
        if (!spans.empty() && x.lo <= spans.back().hi) spans.back().hi = std::max(spans.back().hi, x.lo + x.bytes);
        else { SlotSpan s; s.lo = x.lo; s.hi = x.lo + x.bytes; spans.push_back(s); }
    }
    size_t at = kSlotPad;
    for (SlotSpan& s : spans) {
        at = ((at + 255) & ~(size_t)255) + (size_t)(s.lo & 255);
        s.off = at;
        at += (size_t)(s.hi - s.lo) + kSlotPad;
    }
    if (total) *total = (at + 255) & ~(size_t)255;
    return spans;
}

// the copy lives at `block` (256-byte aligned): every span learns its distance
inline void slot_place(std::vector<SlotSpan>& spans, uintptr_t block)
{
    for (SlotSpan& s : spans) s.delta = (intptr_t)(block + s.off) - (intptr_t)s.lo;
}

// the span that holds address p, or nullptr
inline const SlotSpan* slot_span_of(const std::vector<SlotSpan>& spans, uintptr_t p)
{
    auto it = std::upper_bound(spans.begin(), spans.end(), p, [](uintptr_t v, const SlotSpan& s) { return v < s.lo; });
    if (it == spans.begin()) return nullptr;
    --it;
    return p < it->hi ? &*it : nullptr;
}

inline uintptr_t slot_moved(const std::vector<SlotSpan>& spans, uintptr_t p)
{
    const SlotSpan* s = slot_span_of(spans, p);
    return s ? (uintptr_t)((intptr_t)p + s->delta) : p;
}

// One explicit kernel-argument segment: every aligned 8-byte word whose value lies inside a span moves with that span (a pointer one
// past a span's end, or below its start, does not); trailing bytes that make no whole word are left alone.  Returns the words moved.
// A word that is no pointer but looks like one would move too: the slot proves itself at prerun before it is used (graph_slots.hip).
inline int slot_rebase(unsigned char* args, size_t bytes, const std::vector<SlotSpan>& spans)
{
    int moved = 0;
    for (size_t off = 0; off + 8 <= bytes; off += 8) {
        uint64_t v;
        memcpy(&v, args + off, 8);
        const SlotSpan* s = slot_span_of(spans, (uintptr_t)v);
        if (!s) continue;
        v = (uint64_t)((int64_t)v + (int64_t)s->delta);
        memcpy(args + off, &v, 8);
        moved++;
    }
    return moved;
}

// do [lo, lo + bytes) and any span share a byte?
inline bool slot_touches(const std::vector<SlotSpan>& spans, uintptr_t lo, size_t bytes)
{
    for (const SlotSpan& s : spans)
        if (lo < s.hi && s.lo < lo + bytes) return true;
    return false;
}

}  // namespace tamd
