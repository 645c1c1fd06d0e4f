// Host check of the dependency test behind the barrier-free launches of the direct path (tengine_amd/csrc/graph.h: Access,
// access_of, access_overlap, step_conflict): which steps may run beside each other -- and of what the planners refuse of one step
// (access_of_channels, access_of_bytes, access_of_slot, step_writes_what_it_reads, step_states_nothing).  No device is touched.
// build: hipcc -std=c++17 -I tengine_amd/csrc -I include step_conflict_check.cc -o step_conflict_check
#include <cstdio>

#include "graph.h"

using namespace tamd;

static int bad = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); bad++; } } while (0)

static HTensor dense_u8(char* p, int n, int c, int h, int w)
{
    HTensor t; t.dtype = TAMD_DT_UINT8; t.dims = {n, c, h, w}; t.dptr = p; t.n = n; t.c = c; t.h = h; t.w = w; t.nchw_raw = true; t.cs = 0;
    return t;
}

int main()
{
    static char buf[1 << 20];
    // two dense NCHW tensors side by side, and one that overlaps the first
    HTensor a = dense_u8(buf, 2, 8, 4, 4), b = dense_u8(buf + 256, 2, 8, 4, 4), c = dense_u8(buf + 128, 2, 8, 4, 4);
    EXPECT(access_of(a).size == 256 && access_of(a).period == 0);
    EXPECT(!access_overlap(access_of(a), access_of(b)));
    EXPECT(access_overlap(access_of(a), access_of(c)) && access_overlap(access_of(c), access_of(b)));
    // uint8 concat-by-offset views: channel slices [0,3) and [3,8) of one 8-channel NCHW buffer are disjoint, [2,5) meets both
    HTensor v0 = dense_u8(buf, 2, 3, 4, 4), v1 = dense_u8(buf, 2, 5, 4, 4), v2 = dense_u8(buf, 2, 3, 4, 4);
    v0.is_view = v1.is_view = v2.is_view = true; v0.cs = v1.cs = v2.cs = 8; v0.c_off = 0; v1.c_off = 3; v2.c_off = 2;
    EXPECT(access_of(v0).period == 8 * 16 && access_of(v1).off == 3 * 16 && access_of(v1).len == 5 * 16 && access_of(v0).size == 256);
    EXPECT(!access_overlap(access_of(v0), access_of(v1)));
    EXPECT(access_overlap(access_of(v0), access_of(v2)) && access_overlap(access_of(v1), access_of(v2)));
    EXPECT(access_overlap(access_of(v0), access_of(a)));            // a slice against the whole buffer: conflict
    // int8 NHWC: cs bytes per pixel, a view owns channels [c_off, c_off + c) of every pixel
    HTensor n0; n0.dtype = TAMD_DT_INT8; n0.dims = {2, 16, 4, 4}; n0.dptr = buf; n0.n = 2; n0.c = 16; n0.h = 4; n0.w = 4; n0.cs = 32; n0.is_view = true; n0.c_off = 0;
    HTensor n1 = n0; n1.c_off = 16;
    HTensor whole = n0; whole.is_view = false; whole.c = 32; whole.dims = {2, 32, 4, 4};
    EXPECT(access_of(n0).size == 2u * 16 * 32 && access_of(n0).period == 32 && access_of(n1).off == 16);
    EXPECT(!access_overlap(access_of(n0), access_of(n1)) && access_overlap(access_of(n0), access_of(whole)));
    // a concat input's slot: bytes [off, off + len) of every out_img bytes
    Access s0, s1, s2;
    s0.base = s1.base = s2.base = buf; s0.size = s1.size = s2.size = 2 * 100; s0.period = s1.period = s2.period = 100;
    s0.off = 0; s0.len = 40; s1.off = 40; s1.len = 60; s2.off = 30; s2.len = 20;
    EXPECT(!access_overlap(s0, s1) && access_overlap(s0, s2) && access_overlap(s1, s2));
    // steps: RAW, WAR, WAW and the independent case (two head convolutions reading one map, writing their own tensors)
    Step conv_loc, conv_conf, cat_loc, next;
    HTensor src = dense_u8(buf + 4096, 2, 8, 4, 4), loc = dense_u8(buf + 8192, 2, 4, 4, 4), conf = dense_u8(buf + 12288, 2, 6, 4, 4), out = dense_u8(buf + 16384, 2, 20, 4, 4);
    conv_loc.deps = conv_conf.deps = cat_loc.deps = next.deps = true;
    conv_loc.rd = {access_of(src)}; conv_loc.wr = {access_of(loc)};
    conv_conf.rd = {access_of(src)}; conv_conf.wr = {access_of(conf)};
    cat_loc.rd = {access_of(loc)}; cat_loc.wr = {access_of(out)};
    next.rd = {access_of(conf)}; next.wr = {access_of(src)};         // overwrites what the convolutions read
    EXPECT(!step_conflict(conv_loc, conv_conf) && !step_conflict(conv_conf, conv_loc));       // read-read only
    EXPECT(step_conflict(cat_loc, conv_loc) && step_conflict(conv_loc, cat_loc));             // RAW (either argument order)
    EXPECT(!step_conflict(cat_loc, conv_conf));
    EXPECT(step_conflict(next, conv_loc));                                                    // WAR
    EXPECT(step_conflict(next, conv_conf));                                                   // RAW + WAR
    Step again = conv_loc;
    EXPECT(step_conflict(again, conv_loc));                                                   // WAW
    // a concat input's slot in an NHWC buffer (access_of_channels) against views of the same buffer: a 2x4x4 map, cs = 32
    const Access slot_lo = access_of_channels(whole, 0, 16), slot_hi = access_of_channels(whole, 16, 16), slot_mid = access_of_channels(whole, 8, 16);
    EXPECT(slot_lo.size == 2u * 16 * 32 && slot_lo.period == 32 && slot_hi.off == 16 && slot_hi.len == 16);
    EXPECT(!access_overlap(slot_lo, slot_hi) && !access_overlap(slot_lo, access_of(n1)) && !access_overlap(slot_hi, access_of(n0)));
    EXPECT(access_overlap(slot_lo, access_of(n0)) && access_overlap(slot_hi, access_of(n1)));
    EXPECT(access_overlap(slot_mid, slot_lo) && access_overlap(slot_mid, slot_hi) && access_overlap(slot_mid, access_of(n0)) && access_overlap(slot_mid, access_of(n1)));
    EXPECT(access_overlap(slot_lo, access_of(whole)) && access_overlap(access_of(whole), slot_hi));      // a slot against the whole buffer
    EXPECT(access_of_channels(n1, 0, 16).off == 16);                                                      // counted from the tensor's own first channel
    // one step against itself (what plan_i8 refuses): reading view [0,16) and writing view [16,32) of one buffer is fine (SPP, DenseNet)
    auto none = [](hipStream_t) { return hipSuccess; };
    HTensor d0 = whole, d1 = whole, d2 = whole;                       // three dense NHWC buffers
    d1.dptr = buf + 8192; d2.dptr = buf + 16384;
    const Step spp = make_step("pool", "pool_i8", 0, 0, none, {access_of(n0)}, {access_of(n1)}, false);
    EXPECT(!step_states_nothing(spp) && !step_writes_what_it_reads(spp) && !spp.deps);
    EXPECT(make_step("conv", "k", 0, 0, none, {access_of(d0)}, {access_of(d1)}, true).deps);
    const Step in_place = make_step("add", "eltwise_i8", 0, 0, none, {access_of(d0), access_of(d1)}, {access_of(d0)}, false);
    EXPECT(step_writes_what_it_reads(in_place));
    const Step residual = make_step("conv+add", "k+eltwise", 0, 0, none, {access_of(d0), access_of(d1)}, {access_of(d1)}, false);       // only the SECOND read
    EXPECT(step_writes_what_it_reads(residual));
    EXPECT(!step_writes_what_it_reads(make_step("conv+add", "k+eltwise", 0, 0, none, {access_of(d0), access_of(d1)}, {access_of(d2)}, false)));
    EXPECT(step_writes_what_it_reads(make_step("copy", "concat_copy_i8", 0, 0, none, {access_of(n0)}, {slot_mid}, false)));
    EXPECT(!step_writes_what_it_reads(make_step("copy", "concat_copy_i8", 0, 0, none, {access_of(n0)}, {slot_hi}, false)));
    // a step that states no read or no write "states nothing"
    EXPECT(step_states_nothing(make_step("n", "k", 0, 0, none, {}, {}, false)));
    EXPECT(step_states_nothing(make_step("n", "k", 0, 0, none, {access_of(d0)}, {}, false)));
    EXPECT(step_states_nothing(make_step("n", "k", 0, 0, none, {}, {access_of(d0)}, false)));
    EXPECT(!step_states_nothing(make_step("n", "k", 0, 0, none, {access_of(d0)}, {access_of(d1)}, false)));
    // raw bytes (access_of_bytes): the fp32 copy of a uint8 tensor, the Winograd workspaces.  `copy` holds 2x8x4x4 floats
    HTensor ux = dense_u8(buf + 32768, 2, 8, 4, 4), uy = dense_u8(buf + 36864, 2, 8, 4, 4);
    const Access copy = access_of_bytes(buf + 40960, 256 * sizeof(float));
    EXPECT(copy.base == buf + 40960 && copy.size == 1024 && copy.len == 1024 && copy.period == 0 && copy.off == 0);
    HTensor inside = dense_u8(buf + 40960 + 512, 2, 8, 4, 4), beside = dense_u8(buf + 40960 + 1024, 2, 8, 4, 4);
    EXPECT(access_overlap(copy, access_of(inside)) && access_overlap(access_of(inside), copy));
    EXPECT(!access_overlap(copy, access_of(beside)) && !access_overlap(access_of(beside), copy));
    EXPECT(!access_overlap(copy, access_of(ux)) && !access_overlap(copy, access_of(uy)));
    const Step dequant = make_step("x", "dequant_u8_f32", 0, 0, none, {access_of(ux)}, {copy}, false);
    const Step conv_dma = make_step("conv", "conv_f32_mfma", 0, 0, none, {copy}, {access_of(uy)}, false);
    EXPECT(!step_states_nothing(dequant) && !step_writes_what_it_reads(dequant));
    EXPECT(!step_states_nothing(conv_dma) && !step_writes_what_it_reads(conv_dma));
    EXPECT(step_conflict(dequant, conv_dma) && step_conflict(conv_dma, dequant));               // RAW on the copy
    // a concat input's slot of a DENSE output (access_of_slot): a 2 x (3 + 5) x 4 x 4 channel concat.  At esz = 1 exactly the fields
    // plan_concat_u8 used to build by hand: base y, size y.elems(), period out_img, off, len in_img
    HTensor cat = dense_u8(buf + 65536, 2, 8, 4, 4);
    const size_t out_img = 8 * 16;
    const Access u_lo = access_of_slot(cat, out_img, 0, 3 * 16, 1), u_hi = access_of_slot(cat, out_img, 3 * 16, 5 * 16, 1);
    EXPECT(u_lo.base == buf + 65536 && u_lo.size == 256 && u_lo.period == 128 && u_lo.off == 0 && u_lo.len == 48);
    EXPECT(u_hi.base == buf + 65536 && u_hi.size == 256 && u_hi.period == 128 && u_hi.off == 48 && u_hi.len == 80);
    EXPECT(!access_overlap(u_lo, u_hi));
    // the same concat in fp32
    HTensor catf = cat; catf.dtype = TAMD_DT_FP32;
    const Access f_lo = access_of_slot(catf, out_img, 0, 3 * 16, 4), f_hi = access_of_slot(catf, out_img, 3 * 16, 5 * 16, 4);
    EXPECT(f_lo.base == buf + 65536 && f_lo.size == 1024 && f_lo.period == 512 && f_lo.off == 0 && f_lo.len == 192);
    EXPECT(f_hi.size == 1024 && f_hi.period == 512 && f_hi.off == 192 && f_hi.len == 320);
    EXPECT(!access_overlap(f_lo, f_hi) && !access_overlap(f_hi, f_lo));                           // two slots of one concat: disjoint
    // .. against access_of views of the same buffer: channels [0,3) and [3,8) written in place by their producers
    HTensor fv0 = catf, fv1 = catf;
    fv0.is_view = fv1.is_view = true; fv0.cs = fv1.cs = 8; fv0.c = 3; fv1.c = 5; fv0.c_off = 0; fv1.c_off = 3; fv0.dims = {2, 3, 4, 4}; fv1.dims = {2, 5, 4, 4};
    EXPECT(access_overlap(f_lo, access_of(fv0)) && access_overlap(f_hi, access_of(fv1)));       // the same channels: overlap
    EXPECT(!access_overlap(f_lo, access_of(fv1)) && !access_overlap(f_hi, access_of(fv0)));
    EXPECT(access_overlap(u_lo, access_of(v0)) == false);                                         // (another buffer altogether)
    EXPECT(access_overlap(f_lo, access_of(catf)) && access_overlap(access_of(catf), f_hi));      // a slot against the whole buffer
    EXPECT(access_overlap(u_hi, access_of(cat)));
    printf("step_conflict_check: %d failures\n", bad);
    return bad != 0;
}
