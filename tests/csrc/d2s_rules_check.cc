// depthtospace_refusal (tengine_amd/csrc/node_rules.h) asked on the host, no device involved: one case per line of standard input,
//   dtype has_param const in_quant out_quant block_size xrank x0 .. [orank o0 ..]
// and one line of output per case: "REFUSED <reason>" or "OK r=<r> out=<n,c,h,w> view=<six dims> order=<six axes>".  The dims are copied
// into heap blocks of exactly their size, so that a rule which reads a dimension that is not there is seen by the address sanitizer
// this is built with; the index arithmetic (C / r^2, H * r, W * r, the element count) runs under the undefined-behaviour sanitizer.
#include <stdio.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "node_rules.h"

int main()
{
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        std::string dt;
        int has_param, is_const, in_quant, out_quant, xr;
        tamd_depthtospace_param p;
        memset(&p, 0, sizeof p);
        if (!(in >> dt >> has_param >> is_const >> in_quant >> out_quant >> p.block_size >> xr)) continue;
        std::vector<int> x(xr > 0 ? xr : 0);
        for (int& d : x) in >> d;
        int orank = -1;
        std::vector<int> out;
        if (in >> orank) { out.resize(orank > 0 ? orank : 0); for (int& d : out) in >> d; }
        x.shrink_to_fit(); out.shrink_to_fit();
        const int dtype = dt == "i8" ? TAMD_DT_INT8 : dt == "f32" ? TAMD_DT_FP32 : dt == "f16" ? TAMD_DT_FP16 : TAMD_DT_UINT8;
        tamd::DepthToSpaceGeom g;
        const char* why = tamd::depthtospace_refusal(has_param ? &p : nullptr, dtype, xr, x.data(), is_const != 0, (size_t)in_quant, (size_t)out_quant, orank,
                                                     orank >= 0 ? out.data() : nullptr, &g);
        if (why) { printf("REFUSED %s\n", why); continue; }
        printf("OK r=%d out=%d,%d,%d,%d view=%d,%d,%d,%d,%d,%d order=%d,%d,%d,%d,%d,%d\n", g.r, g.out_dims[0], g.out_dims[1], g.out_dims[2], g.out_dims[3], g.view_dims[0],
               g.view_dims[1], g.view_dims[2], g.view_dims[3], g.view_dims[4], g.view_dims[5], g.order[0], g.order[1], g.order[2], g.order[3], g.order[4], g.order[5]);
    }
    return 0;
}
