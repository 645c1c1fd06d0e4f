// Transpose of a quantised graph (transpose_ref.c), int8 and uint8: the Detect head of the YOLOv5 family, torch's channel shuffle, the
// ONNX form of the SSD head permute, pixel shuffle.  The reference dequantises the input, moves floats and requantises every element,
// so a byte of the output is a function of one byte of the input: the map comes from the host (transpose_tables.cc, built at prerun),
// and these kernels only move bytes.  The geometry is the canonical one of transpose_canon (node_rules.h): at most six (extent, input
// stride) pairs in output order, size-1 axes dropped and neighbours merged, so that a 6-D pixel shuffle and a 2-D matrix are the same
// code.  The source is anything those strides describe -- a dense tensor, or a convolution-stack NHWC buffer read where it lies.
//
// Three forms, chosen by transpose_default_form below (TAMD_PIN=transpose_form=0|1|2 pins one where it is legal):
//   transpose_gather_q8  one thread per output byte, full index arithmetic: legal for every geometry, the cross-check and the A/B baseline
//   transpose_rows_q8    the output's innermost axis has input stride 1: runs of bytes are copied, 16 per lane
//   transpose_tile_q8    the input's stride-1 axis is another output axis: a 64 x 64 tile is exchanged through LDS
//
// The byte map sits in LDS (256 bytes, one coalesced load per block), not in a register per wave behind ds_bpermute_b32 as in lut_u8:
// the bpermute form needs all 64 lanes alive up to the stores, and here lanes are predicated off at the ragged ends of runs and tiles
// and leave early; the tile form needs LDS and its barrier anyway.  IDENT instances take no map at all.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace tamd {

namespace {

__device__ __forceinline__ unsigned map4(const uint8_t* tab, unsigned q)
{
    return (unsigned)tab[q & 0xffu] | (unsigned)tab[(q >> 8) & 0xffu] << 8 | (unsigned)tab[(q >> 16) & 0xffu] << 16 | (unsigned)tab[q >> 24] << 24;
}

// output position -> source offset; *inner / *run: the index along the innermost axis and that axis's extent.  a.nd is uniform and the
// loop is unrolled: the extents and strides are read from the kernel arguments by constant index
__device__ __forceinline__ unsigned src_of(const TransposeArgs& a, unsigned idx, unsigned* inner, unsigned* run)
{
    unsigned src = 0;
#pragma unroll
    for (int d = 5; d >= 0; d--) {
        if (d < a.nd) {
            const unsigned e = (unsigned)a.extent[d];
            const unsigned q = idx / e, r = idx - q * e;
            if (d == a.nd - 1) { *inner = r; *run = e; }
            src += r * (unsigned)a.stride[d];
            idx = q;
        }
    }
    return src;
}

// 16 bytes from s: ONE 16-byte load at any alignment, as slice_u8 and chan_map_u8 take theirs (global loads need no alignment here).  The
// first form of this function took four 4-byte or sixteen byte loads where s was not 16-byte aligned; runs of 85 bytes in 256-byte pixels
// -- the int8 Detect head -- start at every alignment, and the rows form then cost 7.9 us against the gather's 4.9 (profiles/transpose.txt)
__device__ __forceinline__ void load16(const uint8_t* s, unsigned p[4])
{
    __builtin_memcpy(p, s, 16);
}

}  // namespace

// One thread per output byte.
template <bool IDENT>
__global__ __launch_bounds__(256) void transpose_gather_q8(TransposeArgs a)
{
    __shared__ unsigned tab_s[64];
    if (!IDENT) {
        if (threadIdx.x < 64) tab_s[threadIdx.x] = a.table[threadIdx.x];
        __syncthreads();
    }
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab_s);
    const unsigned o = blockIdx.x * 256u + threadIdx.x;
    if (o >= a.total) return;                            // (behind the barrier)
    unsigned inner, run;
    const uint8_t b = a.x[src_of(a, o, &inner, &run)];
    a.y[o] = IDENT ? b : tab[b];
}

// The output's innermost axis has input stride 1, so the output is made of runs of `run` bytes that lie side by side in the source too.
// The whole output is ONE run of a.total bytes cut at the 16-byte boundaries of its address, as slice_u8 cuts an image: thread t owns
// the aligned 16 bytes number t counted from the boundary at or below y, and the bytes [lo, hi) of them belong to the output.  It
// decomposes its first byte once.  A whole chunk inside one source run takes one 16-byte load at whatever address its source has (load16) and
// one 16-byte store; a chunk that crosses runs (runs shorter than 16 bytes: every chunk) walks byte by byte and decomposes again at
// every run's end; the ragged first and last chunks do the same for [lo, hi) and store byte by byte: nothing outside y is touched.
template <bool IDENT>
__global__ __launch_bounds__(256) void transpose_rows_q8(TransposeArgs a)
{
    __shared__ unsigned tab_s[64];
    if (!IDENT) {
        if (threadIdx.x < 64) tab_s[threadIdx.x] = a.table[threadIdx.x];
        __syncthreads();
    }
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab_s);
    const int mis = (int)((uintptr_t)a.y & 15);
    const long L = (long)a.total;
    const long first = ((long)blockIdx.x * 256 + threadIdx.x) * 16 - mis;      // output index of this chunk's byte 0
    const int lo = first < 0 ? (int)-first : 0;
    const int hi = first >= L ? 0 : (L - first >= 16 ? 16 : (int)(L - first));
    if (lo >= hi) return;                                // (behind the barrier)
    unsigned r, R;
    unsigned src = src_of(a, (unsigned)(first + lo), &r, &R);
    const bool whole = lo == 0 && hi == 16;
    unsigned p[4] = {0u, 0u, 0u, 0u};
    if (whole && R - r >= 16) {
        load16(a.x + src, p);
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)                     // (unrolled: registers indexed by constants, no scratch memory)
            if (j >= lo && j < hi) {
                if (r == R) src = src_of(a, (unsigned)(first + j), &r, &R);      // the next run begins
                p[j >> 2] |= (unsigned)a.x[src] << (8 * (j & 3));
                src++; r++;
            }
    }
    if (!IDENT) {
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = map4(tab, p[k]);
    }
    uint8_t* d = a.y + first;
    if (whole) {
        *reinterpret_cast<uint4*>(d) = make_uint4(p[0], p[1], p[2], p[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (j >= lo && j < hi) d[j] = (uint8_t)(p[j >> 2] >> (8 * (j & 3)));
    }
}

// what launch_transpose derives for the tile form: A the output's innermost axis (extent EA, input stride SA), U the input's stride-1
// axis (extent EU, output stride OU), tiles per axis, and the remaining axes -- the grid's batch -- as (extent, input stride, output
// stride), innermost first
struct TransposeTile {
    int EA, SA, EU, OU;
    unsigned TA, TU;
    int nb;
    int bext[4], bin[4], bout[4];
};

__device__ __forceinline__ void transpose4x4(unsigned r0, unsigned r1, unsigned r2, unsigned r3, unsigned o[4])
{
    // rows r0 .. r3 of four bytes each -> o[j] = byte j of r0, r1, r2, r3 (lowest address first): two rounds of byte interleaves
    const unsigned l01 = __builtin_amdgcn_perm(r1, r0, 0x05010400u), h01 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);
    const unsigned l23 = __builtin_amdgcn_perm(r3, r2, 0x05010400u), h23 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
    o[0] = __builtin_amdgcn_perm(l23, l01, 0x05040100u); o[1] = __builtin_amdgcn_perm(l23, l01, 0x07060302u);
    o[2] = __builtin_amdgcn_perm(h23, h01, 0x05040100u); o[3] = __builtin_amdgcn_perm(h23, h01, 0x07060302u);
}

// One wave exchanges a 64 x 64-byte tile over (A, U); the other axes are the grid's batch.
//   in:  tile row al is 64 source bytes along U.  Lane l loads 16 of them, rows (l >> 2) + 16 * rr for rr = 0 .. 3 (four lanes a row: a
//        wave's load is 16 rows of 64 contiguous bytes), maps them and stores them with one ds_write_b128.
//   out: lane l = (u4 = l & 15, a16 = l >> 4) reads the dword column u4 of rows 16 * a16 .. + 15 with sixteen ds_read_b32, transposes
//        four 4 x 4 byte blocks in registers (v_perm_b32) and holds, for each of the four U positions 4 * u4 + j, the 16 bytes along A:
//        four 16-byte stores, a wave's store 16 output rows of 64 contiguous bytes.
// LDS pitch: rows are 64 bytes (16 dwords, whole ds_write_b128 slots), and every GROUP of 16 rows is followed by 64 bytes of padding:
// row al lies at al * 64 + (al >> 4) * 64, a group pitch of 1088 bytes = 272 dwords = 16 (mod 32).  ds_read_b32 banks are (a / 4) % 32
// and conflicts count inside a 32-lane half (cdna_hip_programming.md section 2): in a half the sixteen lanes of one a16 read 16
// consecutive dwords of one row -- banks 16 * (i & 1) .. + 15 for row i of group 0 -- and the sixteen lanes of the other a16 read the
// same row of the next group, 272 dwords on: the other sixteen banks.  No two lanes of a half share a bank; without the padding the
// groups would lie 256 dwords = 0 (mod 32) apart, two-way conflicts on every read.  The writes go to 16 * lane + (64 + 4) * 16 * rr:
// linear in the lane.
// Tiles at the ragged ends of either axis are predicated: a lane outside loads nothing (zeros go to LDS and are never stored), a lane
// across the edge moves its bytes one by one.
template <bool IDENT>
__global__ __launch_bounds__(64) void transpose_tile_q8(TransposeArgs a, TransposeTile t)
{
    __shared__ unsigned tab_s[64];
    __shared__ uint4 tile_s[(64 * 64 + 3 * 64) / 16];
    const int lane = threadIdx.x;
    if (!IDENT) {
        tab_s[lane] = a.table[lane];
        __syncthreads();
    }
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab_s);
    unsigned bid = blockIdx.x;
    const unsigned ta = bid % t.TA; bid /= t.TA;
    const unsigned tu = bid % t.TU; bid /= t.TU;
    unsigned in_base = 0, out_base = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (k < t.nb) {
            const unsigned e = (unsigned)t.bext[k], q = bid / e, r = bid - q * e;
            in_base += r * (unsigned)t.bin[k]; out_base += r * (unsigned)t.bout[k];
            bid = q;
        }
    const int a0 = (int)ta * 64, u0 = (int)tu * 64;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
        const int al = (lane >> 2) + 16 * rr;
        const int ag = a0 + al, ug = u0 + 16 * (lane & 3);
        unsigned p[4] = {0u, 0u, 0u, 0u};
        if (ag < t.EA && ug < t.EU) {
            const uint8_t* s = a.x + in_base + (unsigned)ag * (unsigned)t.SA + (unsigned)ug;
            const int nb = t.EU - ug;
            if (nb >= 16) {
                load16(s, p);
            } else {
#pragma unroll
                for (int j = 0; j < 15; j++)
                    if (j < nb) p[j >> 2] |= (unsigned)s[j] << (8 * (j & 3));
            }
            if (!IDENT) {
#pragma unroll
                for (int k = 0; k < 4; k++) p[k] = map4(tab, p[k]);
            }
        }
        tile_s[al * 4 + (al >> 4) * 4 + (lane & 3)] = make_uint4(p[0], p[1], p[2], p[3]);
    }
    __syncthreads();
    const int u4 = lane & 15, a16 = lane >> 4;
    const unsigned* td = reinterpret_cast<const unsigned*>(tile_s);
    unsigned o[4][4];                                    // o[block of four rows][U position j]
#pragma unroll
    for (int b = 0; b < 4; b++) {
        unsigned r[4];
#pragma unroll
        for (int i = 0; i < 4; i++) r[i] = td[a16 * 272 + (4 * b + i) * 16 + u4];
        transpose4x4(r[0], r[1], r[2], r[3], o[b]);
    }
    const int ag = a0 + 16 * a16;
    if (ag >= t.EA) return;
    const int nb = t.EA - ag;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int ug = u0 + 4 * u4 + j;
        if (ug >= t.EU) continue;
        uint8_t* d = a.y + out_base + (unsigned)ug * (unsigned)t.OU + (unsigned)ag;
        if (nb >= 16 && ((uintptr_t)d & 15) == 0) {
            *reinterpret_cast<uint4*>(d) = make_uint4(o[0][j], o[1][j], o[2][j], o[3][j]);
        } else if (nb >= 16 && ((uintptr_t)d & 3) == 0) {
#pragma unroll
            for (int b = 0; b < 4; b++) reinterpret_cast<unsigned*>(d)[b] = o[b][j];
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (k < nb) d[k] = (uint8_t)(o[k >> 2][j] >> (8 * (k & 3)));
        }
    }
}

bool transpose_form_legal(const TransposeArgs& a, int form)
{
    if (form == kTransposeGather) return true;
    if (form == kTransposeRows) return a.unit == a.nd - 1;
    if (form == kTransposeTile) return a.unit >= 0 && a.unit != a.nd - 1;
    return false;
}

// The default form, decided by the geometry alone, and by what was measured (profiles/transpose.txt): a form becomes the default only
// where it beat the gather beyond the spread.
//  - the tile exchange from 8 MiB on: 36.6 against 38.9 us at 13 MB ((8,3,85,6400) order (0,1,3,2)); at 1.6 MB and 0.4 MB it is behind
//    or inside the spread (7.7 against 5.8 us, 4.4 against 3.9 us) -- a tile is one wave, and a few hundred waves do not hide the
//    load -> LDS -> barrier -> store latency that twenty thousand waves of the gather do.  Where between 1.6 and 13 MB the two cross was
//    not measured; the threshold stands at the lower power of two below the one measured win
//  - the rows form nowhere: 7.6 against 5.0 us on runs of 85 bytes (the int8 Detect head read from NHWC), 3.3 against 3.4 us, inside the
//    spread, on runs of 784 bytes (torch's channel shuffle).  It stays behind TAMD_PIN=transpose_form=1
//  - the gather everywhere else
constexpr unsigned kTransposeTileFromBytes = 8u << 20;
int transpose_default_form(const TransposeArgs& a)
{
    if (a.total >= kTransposeTileFromBytes && transpose_form_legal(a, kTransposeTile)) return kTransposeTile;
    return kTransposeGather;
}

const char* transpose_kernel_name(int form)
{
    return form == kTransposeRows ? "transpose_rows_q8" : form == kTransposeTile ? "transpose_tile_q8" : "transpose_gather_q8";
}

hipError_t launch_transpose(const TransposeArgs& a, hipStream_t s)
{
    if (!a.x || !a.y || (!a.identity && !a.table) || a.nd < 1 || a.nd > 6 || a.total < 1 || a.total > 0x7fffffffu - 64) return hipErrorInvalidValue;
    unsigned long prod = 1, last = 0;
    for (int d = 0; d < a.nd; d++) {
        if (a.extent[d] < 1 || a.stride[d] < 0) return hipErrorInvalidValue;
        prod *= (unsigned long)a.extent[d];
        last += (unsigned long)(a.extent[d] - 1) * (unsigned long)a.stride[d];
        if (prod > a.total || last >= 0x7fffffffu) return hipErrorInvalidValue;
    }
    if (prod != a.total || last >= a.src_bytes) return hipErrorInvalidValue;                       // every read stays inside the source
    if (a.unit >= a.nd || (a.unit >= 0 && a.stride[a.unit] != 1) || !transpose_form_legal(a, a.form)) return hipErrorInvalidValue;
    if (a.form == kTransposeGather) {
        const dim3 grid((a.total + 255) / 256);
        if (a.identity) hipLaunchKernelGGL(transpose_gather_q8<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(transpose_gather_q8<false>, grid, dim3(256), 0, s, a);
    } else if (a.form == kTransposeRows) {
        const unsigned chunks = (a.total + 15) / 16 + 1;     // + 1: an output that starts mid-chunk ends one chunk later
        const dim3 grid((chunks + 255) / 256);
        if (a.identity) hipLaunchKernelGGL(transpose_rows_q8<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(transpose_rows_q8<false>, grid, dim3(256), 0, s, a);
    } else {
        TransposeTile t{};
        const int A = a.nd - 1, U = a.unit;
        t.EA = a.extent[A]; t.SA = a.stride[A]; t.EU = a.extent[U];
        t.TA = (unsigned)(t.EA + 63) / 64; t.TU = (unsigned)(t.EU + 63) / 64;
        unsigned long ostr = 1, blocks = (unsigned long)t.TA * t.TU;
        for (int d = a.nd - 1; d >= 0; d--) {                // output strides: the product of the extents behind an axis
            if (d == U) t.OU = (int)ostr;
            else if (d != A) {
                t.bext[t.nb] = a.extent[d]; t.bin[t.nb] = a.stride[d]; t.bout[t.nb] = (int)ostr;
                t.nb++;
                blocks *= (unsigned long)a.extent[d];
            }
            ostr *= (unsigned long)a.extent[d];
        }
        if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
        const dim3 grid((unsigned)blocks);
        if (a.identity) hipLaunchKernelGGL(transpose_tile_q8<true>, grid, dim3(64), 0, s, a, t);
        else hipLaunchKernelGGL(transpose_tile_q8<false>, grid, dim3(64), 0, s, a, t);
    }
    return hipGetLastError();
}

}  // namespace tamd
