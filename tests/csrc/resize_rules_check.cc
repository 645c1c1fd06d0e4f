// resize_refusal (tengine_amd/csrc/node_rules.h) asked on the host, no device involved, with the two builders it calls
// (csrc/resize_tables.cc, csrc/interp_tables.cc) linked in: one case per line of standard input,
//   dtype has_param const in_quant out_quant scale_h scale_w type in_scale in_zp out_scale out_zp xrank x0 .. [orank o0 ..]
// (the four floats as the hexadecimal bit pattern of a float, so that nothing depends on a decimal conversion; in_scale 0: the caller
// has no quantisation values) and one line of output per case: "REFUSED <reason>" or
// "OK out=<n,c,h,w> sh=<sh> sw=<sw> iy=<..> ix=<..> table=<crc>", the table as the sum of entry * (index + 1).
// The dims are copied into heap blocks of exactly their size, so that a rule which reads a dimension that is not there is seen by the
// address sanitizer this is built with; the float-to-int conversions of the shape rule, the index rule and the table run under the
// undefined-behaviour sanitizer.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "node_rules.h"

static float bits(const std::string& hex)
{
    const unsigned u = (unsigned)strtoul(hex.c_str(), nullptr, 16);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main()
{
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        std::string dt, sh, sw, is, os;
        int has_param, is_const, in_quant, out_quant, xr;
        tamd_resize_param p;
        tamd::ResizeQuant q;
        memset(&p, 0, sizeof p);
        if (!(in >> dt >> has_param >> is_const >> in_quant >> out_quant >> sh >> sw >> p.type >> is >> q.in_zp >> os >> q.out_zp >> xr)) continue;
        p.scale_h = bits(sh); p.scale_w = bits(sw); q.in_scale = bits(is); q.out_scale = bits(os);
        std::vector<int> x(xr > 0 ? xr : 0);
        for (int& d : x) in >> d;
        int orank = -1;
        std::vector<int> out;
        if (in >> orank) { out.resize(orank > 0 ? orank : 0); for (int& d : out) in >> d; }
        x.shrink_to_fit(); out.shrink_to_fit();
        const int dtype = dt == "i8" ? TAMD_DT_INT8 : dt == "f32" ? TAMD_DT_FP32 : dt == "f16" ? TAMD_DT_FP16 : TAMD_DT_UINT8;
        tamd::ResizeGeom g;
        const char* why = tamd::resize_refusal(has_param ? &p : nullptr, dtype, xr, x.data(), is_const != 0, (size_t)in_quant, (size_t)out_quant,
                                               q.in_scale != 0.f ? &q : nullptr, orank, orank >= 0 ? out.data() : nullptr, &g);
        if (why) { printf("REFUSED %s\n", why); continue; }
        unsigned long crc = 0;
        for (int b = 0; b < 256; b++) crc += (unsigned long)g.table[b] * (unsigned long)(b + 1);
        printf("OK out=%d,%d,%d,%d sh=%d sw=%d iy=", g.out_dims[0], g.out_dims[1], g.out_dims[2], g.out_dims[3], g.sh, g.sw);
        for (size_t i = 0; i < g.iy.size(); i++) printf("%s%d", i ? "," : "", g.iy[i]);
        printf(" ix=");
        for (size_t i = 0; i < g.ix.size(); i++) printf("%s%d", i ? "," : "", g.ix[i]);
        printf(" table=%lu\n", g.have_table ? crc : 0ul);
    }
    return 0;
}
