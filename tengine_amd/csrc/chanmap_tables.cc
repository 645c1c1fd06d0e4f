// The host-built operands of the channel-moving operators of quantised graphs: Split (split_ref.c) and ShuffleChannel
// (shuffle_channel_ref.c).  In the reference the int8 Split (:109-135) and ShuffleChannel in every type are memcpys: no quantisation
// parameter is read and -128 stays -128.  The uint8 Split alone requantises (:94-99), one byte to one byte.  So the device keeps no
// formula: which input channel an output channel takes, and the uint8 byte map, are built here at prerun and the kernels
// (chanmap.hip) only move bytes.
//
// Plain C++ (no HIP), compiled with -ffp-contract=off (build.py): the ONE contraction the reference's compiled code makes is written
// out as fmaf below, nothing else may fuse.  The file links alone (tests/csrc/chanmap_tables_check.cc runs it under the sanitizers).
#include "chanmap_tables.h"

#include <math.h>

extern "C" int tamd_shuffle_sources(int channels, int group, int* src)
{
    if (!src || channels < 1 || group < 1 || channels % group != 0) return -1;
    const int per = channels / group;                        // shuffle_channel_ref.c: chs_per_group
    for (int i = 0; i < group; i++)
        for (int j = 0; j < per; j++) src[group * j + i] = per * i + j;
    return 0;
}

extern "C" int tamd_split_table(float in_scale, int in_zp, float out_scale, int out_zp, unsigned char table[256])
{
    if (!table) return -1;
    const float rescale = in_scale / out_scale;              // split_ref.c:76
    for (int b = 0; b < 256; b++) {
        // :94  int udata = roundf((input_data[i] - input_zero) * rescale + output_zero);  the difference is an int, converted once; the
        // product and the sum are ONE fused operation in the reference's object code (vfmadd132ss in ref_split_uint8)
        const float r = roundf(fmaf((float)(b - in_zp), rescale, (float)out_zp));
        int v = r >= 2147483648.f || r < -2147483648.f || r != r ? (int)0x80000000 : (int)r;      // cvttss2si: out of range, NaN -> INT_MIN
        if (v > 255) v = 255;
        else if (v < 0) v = 0;
        table[b] = (unsigned char)v;
    }
    return 0;
}
