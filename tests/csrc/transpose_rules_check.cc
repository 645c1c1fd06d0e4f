// transpose_refusal (tengine_amd/csrc/node_rules.h) asked on the host, no device involved: one case per line of standard input,
//   dtype const in_quant out_quant rank d0 .. d(rank-1) len o0 .. o(len-1) [out_rank e0 ..]
// and one line of output per case: "REFUSED <reason>" or "OK out=<dims> geom=<extent>:<stride>,.. unit=<axis>".  len -1: no parameter.
// The quantisation values are fixed (0.05 / 3 -> 0.04 / 5), "bad" as dtype gives parameters no table can be built for.
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
        int is_const, in_quant, out_quant, rank, len;
        if (!(in >> dt >> is_const >> in_quant >> out_quant >> rank)) continue;
        std::vector<int> dims(rank > 0 ? rank : 0);
        for (int& d : dims) in >> d;
        in >> len;
        tamd_transpose_param p;
        memset(&p, 0, sizeof p);
        p.dim_num = len;
        for (int i = 0; i < len; i++) { int o; in >> o; if (i < 8) p.order[i] = o; }
        int out_rank = -1;
        std::vector<int> out_dims;
        if (in >> out_rank) { out_dims.resize(out_rank); for (int& d : out_dims) in >> d; }
        const bool bad = dt == "bad";
        const int dtype = dt == "i8" ? TAMD_DT_INT8 : dt == "f32" ? TAMD_DT_FP32 : TAMD_DT_UINT8;
        tamd::TransposeGeom g;
        unsigned char table[256];
        const char* why = tamd::transpose_refusal(len < 0 ? nullptr : &p, dtype, rank, dims.data(), is_const != 0, (size_t)in_quant, bad ? 1.0f : 0.05f, 3, (size_t)out_quant,
                                                  bad ? 1e-8f : 0.04f, 5, out_rank, out_rank >= 0 ? out_dims.data() : nullptr, &g, table);
        if (why) { printf("REFUSED %s\n", why); continue; }
        printf("OK out=");
        for (int i = 0; i < g.rank; i++) printf("%s%d", i ? "," : "", g.out_dims[i]);
        printf(" geom=");
        for (int i = 0; i < g.nd; i++) printf("%s%d:%ld", i ? "," : "", g.extent[i], g.stride[i]);
        printf(" unit=%d\n", g.unit);
    }
    return 0;
}
