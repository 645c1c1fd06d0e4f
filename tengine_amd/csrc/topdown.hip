// The top-down merge of a feature pyramid in a uint8 graph (RetinaFace's neck): nearest Interp -> Crop -> same-shape Eltwise as ONE
// launch.  The three reference nodes (interp_ref.c:384-410, crop_ref.c:147-253, eltwise_ref.c:311-585) make of every output byte
//   u = T[small[n][c][iy[h + h0]][ix[w + w0]]]     T: the Interp's byte map; the Crop copies raw bytes, it only moves the indices
//   y = requant(deq(u) op deq(lateral))             the chain of eltwise_u8_k, u dequantised with the Crop OUTPUT's parameters
// so the up-sampled map and its cut are never written: the launch reads the small map (a quarter of the output's bytes, and every
// byte of it four times out of the L1) and the lateral, and writes the merge.  T, iy and ix come from the host (interp_tables.cc), the
// two index vectors already shifted and cut by the Crop's box (graph_plan_maps.hip: plan_topdown_u8).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "u8_epilogue.h"

namespace tamd {

constexpr int kTopdownIxLds = 512;                       // output columns whose index vector a block stages in LDS (2 KiB)

// Dense NCHW, all three tensors.  The lateral and the output have the same dims and are 16-byte aligned (launch_topdown_u8 checks it),
// so a lane owns the aligned 16-byte chunk number t of the TENSOR, as in chan_gate_u8: one 16-byte load of the lateral, one 16-byte
// store, and the chunk may straddle rows and planes (W = 19, H * W = 285).  The lane divides its first byte into (plane, row, column)
// once; the row index iy[h] is read once per row segment -- a chunk of a map at least 16 wide holds at most two, found up front; a
// narrower map walks its bytes as the reference's loops do and reads it when the walk enters a row -- and the column indices come from
// LDS (IXLDS: OW <= kTopdownIxLds; wider maps read them from memory).  Only the last chunk of the tensor can be ragged: it loads and
// stores byte by byte and touches nothing behind the tensor's last byte.
// The byte map lives in registers, one dword per lane, looked up with ds_bpermute (interp.hip, lut_u8): bpermute reads 0 from a disabled
// lane and the requantisation's hand-over test is a wave-level ballot, so NO THREAD LEAVES EARLY -- a lane behind the tensor's end
// loads nothing, computes on zeros and stores nothing.  IDENT: the map is the identity, no lookups.
// Blocks of ONE wave, as interp_nearest_u8: a lane carries 16 bytes, and a neck-sized merge (1 x 64 x 15 x 20) is 1200 lanes.
template <bool IDENT, bool IXLDS>
__global__ __launch_bounds__(64) void topdown_u8_kernel(TopdownU8Args a)
{
    __shared__ int ix_s[IXLDS ? kTopdownIxLds : 1];
    const unsigned tab = IDENT ? 0u : a.table[threadIdx.x & 63];
    if (IXLDS) {
        for (int i = threadIdx.x; i < a.OW; i += 64) ix_s[i] = a.ix[i];
        __syncthreads();
    }
    const int OHW = a.OH * a.OW;
    const int total = (int)a.planes * OHW;                                             // (fits: launch_topdown_u8) -- positions in 32-bit divisions
    const int first = (int)(blockIdx.x * 64 + threadIdx.x) * 16;                       // tensor index of this chunk's byte 0
    const int hi = first >= total ? 0 : (total - first >= 16 ? 16 : total - first);
    unsigned pu[4] = {0u, 0u, 0u, 0u}, pl[4] = {0u, 0u, 0u, 0u};
    if (hi > 0) {
        int plane = first / OHW;
        const int rem = first - plane * OHW;
        int oy = rem / a.OW, ox = rem - oy * a.OW;
        if (hi == 16 && a.OW >= 16) {
            // a whole chunk with at most ONE row boundary inside it: both source rows are found first (two index loads that depend on
            // nothing), then the sixteen gathers depend on their own column index alone and are all in flight together, as in
            // interp_nearest_u8 (the stepping loop below chains every load behind the position of the byte before it)
            const bool last = oy + 1 == a.OH;            // the next row opens the next plane (behind the last one: computed, never read)
            const uint8_t* row0 = a.small + ((size_t)plane * a.H + a.iy[oy]) * a.W;
            const uint8_t* row1 = a.small + ((size_t)(plane + (last ? 1 : 0)) * a.H + a.iy[last ? 0 : oy + 1]) * a.W;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int o = ox + j;
                const bool wrap = o >= a.OW;
                const int col = wrap ? o - a.OW : o;
                pu[j >> 2] |= (unsigned)(wrap ? row1 : row0)[IXLDS ? ix_s[col] : a.ix[col]] << (8 * (j & 3));
            }
        } else {
            const uint8_t* row = a.small + ((size_t)plane * a.H + a.iy[oy]) * a.W;
#pragma unroll
            for (int j = 0; j < 16; j++)                 // (unrolled: registers indexed by constants, no scratch memory)
                if (j < hi) {
                    pu[j >> 2] |= (unsigned)row[IXLDS ? ix_s[ox] : a.ix[ox]] << (8 * (j & 3));
                    if (++ox == a.OW) {
                        ox = 0;
                        if (++oy == a.OH) { oy = 0; plane++; }
                        row = a.small + ((size_t)plane * a.H + a.iy[oy]) * a.W;      // (behind the tensor's last byte: computed, never read)
                    }
                }
        }
        if (hi == 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(a.lat + first);
            pl[0] = v.x; pl[1] = v.y; pl[2] = v.z; pl[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++)
                if (j < hi) pl[j >> 2] |= (unsigned)a.lat[first + j] << (8 * (j & 3));
        }
    }
    const float inv = __fdiv_rn(1.0f, a.out_scale);
    unsigned out[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        unsigned m = pu[d];
        if (!IDENT) {
            m = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const unsigned q = (pu[d] >> (8 * b)) & 0xffu;
                const unsigned t = (unsigned)__builtin_amdgcn_ds_bpermute((int)(q & 0xfcu), (int)tab);      // byte address of lane q >> 2
                m |= ((t >> (8 * (q & 3u))) & 0xffu) << (8 * b);
            }
        }
        float r[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const float fu = (float)((int)((m >> (8 * b)) & 0xffu) - a.zu) * a.su;
            const float fl = (float)((int)((pl[d] >> (8 * b)) & 0xffu) - a.zl) * a.sl;
            const float fa = a.u_first ? fu : fl, fb = a.u_first ? fl : fu;          // the operands stay in the node's order: SUB shows it
            switch (a.type) {
            case 0: r[b] = fa * fb; break;
            case 2: r[b] = fa + fb; break;
            case 4: r[b] = fa - fb; break;
            default: r[b] = fa > fb ? fa : fb; break;
            }
        }
        int q4[4];
        quant_round_sat_u8_w4(r, a.out_scale, inv, a.out_zp, q4);                    // == quant_round_sat_u8_w of each, one ballot for the four
        out[d] = (unsigned)q4[0] | (unsigned)q4[1] << 8 | (unsigned)q4[2] << 16 | (unsigned)q4[3] << 24;
    }
    if (hi == 16) {
        *reinterpret_cast<uint4*>(a.y + first) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (j < hi) a.y[first + j] = (uint8_t)(out[j >> 2] >> (8 * (j & 3)));
    }
}

hipError_t launch_topdown_u8(const TopdownU8Args& a, hipStream_t s)
{
    if (!a.small || !a.lat || !a.y || !a.iy || !a.ix || (!a.identity && !a.table)) return hipErrorInvalidValue;
    if (a.planes < 1 || a.H < 1 || a.W < 1 || a.OH < 1 || a.OW < 1) return hipErrorInvalidValue;
    if (a.type != 0 && a.type != 2 && a.type != 4 && a.type != 6) return hipErrorInvalidValue;
    if (((uintptr_t)a.lat | (uintptr_t)a.y) & 15) return hipErrorInvalidValue;
    if ((long)a.OH * a.OW > 0x7fffffffL || (long)a.H * a.W > 0x7fffffffL) return hipErrorInvalidValue;
    const long total = a.planes * ((long)a.OH * a.OW);
    if (total > 0x7fffffffL - 64 * 16 || a.planes * ((long)a.H * a.W) > 0x7fffffffL) return hipErrorInvalidValue;      // the kernel counts bytes in 32 bits
    const long blocks = ((total + 15) / 16 + 63) / 64;
    const dim3 grid((unsigned)blocks);
    const bool lds = a.OW <= kTopdownIxLds;
    if (a.identity) {
        if (lds) hipLaunchKernelGGL((topdown_u8_kernel<true, true>), grid, dim3(64), 0, s, a);
        else hipLaunchKernelGGL((topdown_u8_kernel<true, false>), grid, dim3(64), 0, s, a);
    } else {
        if (lds) hipLaunchKernelGGL((topdown_u8_kernel<false, true>), grid, dim3(64), 0, s, a);
        else hipLaunchKernelGGL((topdown_u8_kernel<false, false>), grid, dim3(64), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace tamd
