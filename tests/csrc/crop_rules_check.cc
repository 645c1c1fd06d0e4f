// crop_refusal (tengine_amd/csrc/node_rules.h) asked on the host, no device involved: one case per line of standard input,
//   dtype has_param inputs const in_quant out_quant xrank x0 .. lrank l0 .. num_args offset_c offset_h offset_w crop_h crop_w center_crop axis flag [orank o0 ..]
// and one line of output per case: "REFUSED <reason>" or "OK start=<n,c,h,w> out=<n,c,h,w>".  The dims are copied into heap blocks of
// exactly their size, so that a rule which reads a dimension that is not there is seen by the address sanitizer this is built with.
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
        int has_param, inputs, is_const, in_quant, out_quant, xr, lr;
        if (!(in >> dt >> has_param >> inputs >> is_const >> in_quant >> out_quant >> xr)) continue;
        std::vector<int> x(xr > 0 ? xr : 0);
        for (int& d : x) in >> d;
        in >> lr;
        std::vector<int> like(lr > 0 ? lr : 0);
        for (int& d : like) in >> d;
        tamd_crop_param p;
        memset(&p, 0, sizeof p);
        in >> p.num_args >> p.offset_c >> p.offset_h >> p.offset_w >> p.crop_h >> p.crop_w >> p.center_crop >> p.axis >> p.flag;
        int orank = -1;
        std::vector<int> out;
        if (in >> orank) { out.resize(orank > 0 ? orank : 0); for (int& d : out) in >> d; }
        x.shrink_to_fit(); like.shrink_to_fit(); out.shrink_to_fit();
        const int dtype = dt == "i8" ? TAMD_DT_INT8 : dt == "f32" ? TAMD_DT_FP32 : TAMD_DT_UINT8;
        tamd::CropGeom g;
        const char* why = tamd::crop_refusal(has_param ? &p : nullptr, dtype, inputs, xr, x.data(), is_const != 0, (size_t)in_quant, lr, like.data(), (size_t)out_quant, orank,
                                             orank >= 0 ? out.data() : nullptr, &g);
        if (why) { printf("REFUSED %s\n", why); continue; }
        printf("OK start=%d,%d,%d,%d out=%d,%d,%d,%d\n", g.start[0], g.start[1], g.start[2], g.start[3], g.out_dims[0], g.out_dims[1], g.out_dims[2], g.out_dims[3]);
    }
    return 0;
}
