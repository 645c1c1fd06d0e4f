// chan_lut_u8: a byte map per channel over a dense uint8 tensor [N][C][HW] -- the uint8 BatchNorm (batchnorm_kernel_ref_uint8.c:40-107
// is a function of one byte and its channel; tamd_batchnorm_table builds the C maps on the host).
//
// prelu_u8 (prelu.hip) applies the same [C][64] tables with a block per plane and walks ragged plane ends byte-wise
// (profiles/prelu_ops.txt names both as its weaknesses): on the [N,128] output of a face model's last FullyConnected that is 128 blocks
// for 128 bytes.  This kernel is chunk-owned, like chan_gate_u8: a lane owns the aligned 16-byte chunk k of the output, bytes
// [16k, 16k + 16).  Both tensors own their buffers and are 16-byte aligned, so the tensor has no ragged head; the one ragged chunk is
// the LAST, and only its lane takes the byte-wise path.  Nothing outside [0, total) is read or written.
//  - one 16-byte load; the channel of the chunk's first byte from ONE division pair (plane = i / HW, c = plane % C, rem = i % HW),
//    then carries: rem + 1 == HW moves to the next channel, c + 1 == C back to 0.  For HW = 1 that is c = i % C and a carry per byte
//  - sixteen look-ups tables[c][b], one 16-byte store
// Where the tables live -- the one design decision: in GLOBAL memory, read through the vector L1 / L2, not staged in LDS.  A block of
// 256 lanes maps 4 KiB; staging C * 256 bytes (32 KiB at C = 128, over a block's LDS share from C = 256 on) would cost every block a
// copy eight times the bytes it maps, and one-block tensors ([1,128]: 128 bytes) would pay 32 KiB for 128 look-ups.  From global
// memory a lane touches only the lines it needs: with HW >= 16 a wave's 1024 bytes span at most a few channels (a few 256-byte
// maps, L1 hits after the first lane), with HW = 1 every byte has its own channel and the C maps (32 KiB at C = 128) sit in L2 and, up
// to its 32 KiB, in the L1.  ds_bpermute cannot serve: it moves a dword per lane between 64 lanes, 256 bytes of table, ONE channel --
// lut_u8's trick, which a per-channel map outgrows as soon as a wave spans two channels.  The LDS form was not built and not measured.
// Measured against the per-plane form and lut_u8 on the same bytes (profiles/bytemap_chains.txt): 3.0 us from 128 bytes to 200 KB, under
// lut_u8's 3.3 - 3.4 us (whose LDS table costs every block a staging step) and ahead of prelu_u8 on [32,128] and on planes below 784 bytes.
#include "kernels.h"

namespace tamd {

__global__ __launch_bounds__(256) void chan_lut_u8_kernel(ChanLutU8Args a)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i0 = k * 16;
    if (i0 >= a.total) return;
    const unsigned char* tab = reinterpret_cast<const unsigned char*>(a.tables);
    const size_t plane = i0 / (size_t)a.HW;
    int rem = (int)(i0 - plane * (size_t)a.HW);
    int c = (int)(plane % (size_t)a.C);
    if (i0 + 16 <= a.total) {
        const uint4 v = *reinterpret_cast<const uint4*>(a.x + i0);
        const unsigned in[4] = {v.x, v.y, v.z, v.w};
        unsigned out[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            unsigned o = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned b = (in[d] >> (8 * j)) & 255u;
                o |= (unsigned)tab[(size_t)c * 256 + b] << (8 * j);
                if (++rem == a.HW) { rem = 0; if (++c == a.C) c = 0; }
            }
            out[d] = o;
        }
        *reinterpret_cast<uint4*>(a.y + i0) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {                                                         // the tensor's ragged tail: the last lane alone, byte by byte
        for (size_t i = i0; i < a.total; i++) {
            a.y[i] = tab[(size_t)c * 256 + a.x[i]];
            if (++rem == a.HW) { rem = 0; if (++c == a.C) c = 0; }
        }
    }
}

hipError_t launch_chan_lut_u8(const ChanLutU8Args& a, hipStream_t s)
{
    if (!a.x || !a.y || !a.tables || a.C < 1 || a.HW < 1 || a.total < 1 || a.total % ((size_t)a.C * a.HW)) return hipErrorInvalidValue;
    if (((uintptr_t)a.x | (uintptr_t)a.y | (uintptr_t)a.tables) & 15) return hipErrorInvalidValue;
    const size_t chunks = (a.total + 15) / 16, blocks = (chunks + 255) / 256;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(chan_lut_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace tamd
