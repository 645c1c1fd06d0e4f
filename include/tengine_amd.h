/*
 * tengine_amd.h -- C ABI of the MI355X (gfx950) device backend for Tengine's quantised CNN hot path.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only; no C++/torch types.  Every entry
 * point names the reference interface it replaces (paths relative to the reference root):
 *
 *   reference (source/device/device.h:40-108)          this library
 *   ---------------------------------------------------------------------------------------------
 *   interface.init / release_device                     tamd_init / tamd_shutdown
 *   serializer load_mem  (tm2_serializer.c:915-936)     tamd_graph_load_tm2        (same tmfile bytes)
 *   create_graph_node/tensor (c_api.c)                  tamd_graph_add_tensor / tamd_graph_add_node
 *   allocator.describe (cuda_device.cc:47-83)           tamd_op_supported
 *   interface.pre_run  (scheduler.c:49-59)              tamd_graph_prerun
 *   interface.run      (scheduler.c:134)                tamd_graph_run  (host in -> H2D -> launches -> D2H)
 *   interface.async_run / async_wait (device.h:60-63)   tamd_graph_run_async / tamd_graph_wait
 *   interface.post_run / release_graph                  tamd_graph_destroy
 *   set_tensor_buffer / get_tensor_buffer (c_api.c)     tamd_graph_set_input / tamd_graph_get_output
 *
 * The Tengine device plugin (tengine_amd/device/hip_device.cc -> register_hip_device(), the
 * symbol name cmake/registry.cmake:11-31 derives from `hip_device.cc`) is a thin translator from
 * `struct subgraph` onto this ABI; see INTEGRATION.md.
 *
 * Conventions follow the reference: every int function returns 0 on success, a negative value on
 * failure (c_api.c:463-497); tamd_last_error() gives the message.  Tensors cross the boundary in
 * the reference's layouts (activations NCHW, conv weights OIHW, FC weights [out][hidden], int32
 * bias, per-tensor activation scales, per-out-channel weight scales); the NHWC / MFMA-packed device
 * layouts are private to the backend.
 */
#ifndef TENGINE_AMD_H
#define TENGINE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAMD_API __attribute__((visibility("default")))

/* data types == TENGINE_DT_* (source/api/c_api.h:58-63) */
enum { TAMD_DT_FP32 = 0, TAMD_DT_FP16 = 1, TAMD_DT_INT8 = 2, TAMD_DT_UINT8 = 3, TAMD_DT_INT32 = 4 };
/* tensor types == TENSOR_TYPE_* (c_api.h:70-74) */
enum { TAMD_TT_VAR = 1, TAMD_TT_CONST = 2, TAMD_TT_INPUT = 3 };

/* operator codes of this ABI (the plugin maps OP_* of source/operator/op.h:38-145 onto these;
 * the tm2 loader maps TM2_OPTYPE_* of tm2_format.h:157-264) */
enum {
    TAMD_OP_INPUT = 0,
    TAMD_OP_CONST = 1,
    TAMD_OP_CONV = 2,    /* param: tamd_conv_param  */
    TAMD_OP_FC = 3,      /* param: tamd_fc_param    */
    TAMD_OP_POOL = 4,    /* param: tamd_pool_param  */
    TAMD_OP_RELU = 5,    /* param: tamd_relu_param  */
    TAMD_OP_ELTWISE = 6, /* param: tamd_eltwise_param; PROD 0 / SUM 2 / SUB 4 / MAX 6 of two tensors of one shape in every graph type; in
                          * int8 / uint8 graphs also the channel gate of a Squeeze-and-Excitation block, x (N,C,H,W) op gate (N,C,1,1) for
                          * PROD / SUM / SUB -- always x op gate, the gate may be listed first at batch 1 (eltwise_ref.c); the output has
                          * x's dims.  In int8 / uint8 graphs also, by a 256-entry table and one lut_u8 launch (tamd_eltwise_table):
                          *  - the scalar form, inputs [x, c]: x a 4-D activation, c a CONSTANT of one element listed second (uint8 graphs:
                          *    a uint8 or an fp32 constant; int8 graphs: an int8 one); PROD 0, PROD_SCALAR 1, SUM 2, SUB 4, SUB_SCALAR 5,
                          *    MIN_SCALAR 8, DIV 10
                          *  - the unary form, one input, 4-D: RSQRT 7, LOG 11, EXP 12, SQRT 13, FLOOR 14, SQUARE 15, POWER 17 (shift, scale,
                          *    power)
                          * MAX with a gate or a scalar, a gate of another shape, a one-element operand that is no constant or is listed
                          * first, SUM_SCALAR 3, LAST 9, POW 16, and a node whose table holds a value the reference cannot convert to int
                          * are refused by name (tamd_node_supported answers 0) */
    TAMD_OP_CONCAT = 7,  /* param: tamd_concat_param */
    TAMD_OP_DROPOUT = 8, /* identity */
    TAMD_OP_UPSAMPLE = 9,/* param: tamd_upsample_param; nearest, an integer factor >= 1; fp32 / uint8 graphs, and int8 graphs for a 4-D
                          * tensor: upsample_ref.c:162-165 runs its uint8 routine on the int8 BYTES (0 .. 255), and so does the device */
    TAMD_OP_RELU6 = 10,
    TAMD_OP_FLATTEN = 11,
    TAMD_OP_SOFTMAX = 12, /* param: tamd_softmax_param (NULL: axis 1); fp32 / uint8 graphs: any axis; int8 graphs: any axis >= 1 of a
                           * 2-D / 3-D / 4-D tensor, <= 16000 values along it (softmax_kernel_ref_int8.c:41-117; the spatial axes of an
                           * NHWC tensor and the axes of a dense tensor since round 6)                                               */
    TAMD_OP_PERMUTE = 13, /* param: tamd_permute_param; uint8 and (round 6) int8 graphs, order (0,2,3,1) -- the SSD head permute */
    TAMD_OP_RESHAPE = 14, /* param: tamd_reshape_param; a view of a dense tensor (uint8 / fp32 graphs; int8 since round 6: what a
                           * Permute / Flatten / Reshape / PriorBox / flat Concat produces is dense on the device)                  */
    TAMD_OP_PRIORBOX = 15,/* param: tamd_priorbox_param; uint8 / fp32 and (round 6) int8 graphs, batch 1.  Depends on shapes only:
                           * evaluated ONCE at prerun (priorbox_ref.c:53-213 re-computes the same numbers at every run), no launch   */
    /* the byte-to-byte activations of quantised graphs: each is, in the reference, a function of ONE input byte and the two tensors'
     * quantisation parameters, so the device maps bytes through a 256-entry table built at prerun (tamd_lut_table, csrc/lut_tables.cc)
     * with one kernel, lut_u8.  int8 / uint8 graphs only; fp32 graphs keep these four on the CPU device */
    TAMD_OP_SIGMOID = 16,  /* int8 / uint8 (sigmoid_ref.c:84-170)                                                                  */
    TAMD_OP_CLIP = 17,     /* param: tamd_clip_param; int8 / uint8 (clip_kernel_ref_int8.c / _uint8.c:41-80); ReLU6 of an ONNX export */
    TAMD_OP_HARDSWISH = 18,/* param: tamd_hardswish_param; uint8 only (hardswish_kernel_ref_uint8.c:41-83; no int8 kernel in the reference) */
    TAMD_OP_MISH = 19,     /* uint8 only, a 4-D tensor (mish_kernel_ref_uint8.c:41-95 reads dims[0..3]; no int8 kernel in the reference)  */
    /* every ONNX Resize: param tamd_interp_param.  Nearest (resize_type 1) of a 4-D tensor in int8 / uint8 graphs: any batch, scales
     * below 1, non-integer and per-axis scales (interp_ref.c:275-301 / :384-410).  The source indices (tamd_interp_indices) and the byte
     * map (tamd_interp_table) are built on the host at prerun.  Bilinear and fp32 graphs stay on the CPU device */
    TAMD_OP_INTERP = 20,
    /* 21: reserved, never supported */
    /* the channel-moving operators of a ShuffleNet unit, int8 / uint8 graphs: in the reference both are byte copies (split_ref.c:109-135,
     * shuffle_channel_ref.c), only the uint8 Split requantises byte to byte (tamd_split_table).  fp32 graphs keep them on the CPU device */
    TAMD_OP_SPLIT = 22,          /* param: tamd_split_param; the split_sizes form along the channel axis of a 4-D tensor */
    TAMD_OP_SHUFFLECHANNEL = 23, /* param: tamd_shufflechannel_param; a 4-D tensor, channels % group == 0, any batch */
    /* 24: reserved, never supported */
    /* the activation of MobileFaceNet and the ArcFace / RetinaFace family, int8 / uint8 graphs: no param; inputs [data, slope].  A 4-D
     * data tensor; the slope is a constant TAMD_DT_FP16 tensor of one value per channel (uint8: or one value for all), which the
     * reference widens with its own routine -- not IEEE: every exact power of two (0.25, 1, ...) widens to +0, so such a PReLU is a
     * ReLU (tamd_prelu_slope).  prelu_ref.c:160-384; int8 saturates at +-127.  fp32 graphs keep the node on the CPU device */
    TAMD_OP_PRELU = 25,
    /* YOLOv4-tiny's routes (darknet "route groups=2 group_id=1") and the x[..., ::2, ::2] of YOLOv5's Focus, uint8 graphs: param
     * tamd_slice_param.  The onnx form with one output on a 4-D tensor: any axis, any batch, step >= 1 (slice_ref.c:229-291); the
     * reference dequantises, copies floats and requantises byte to byte (tamd_slice_table), and copies the bytes as they are when the
     * output has the input's dims.  The caffe, mxnet and tf forms, int8 graphs (no kernel in the reference) and fp32 graphs stay on
     * the CPU device */
    TAMD_OP_SLICE = 26,
    /* every ONNX Transpose -- the Detect head of the YOLOv5 family ((0,1,3,4,2) behind a Reshape), torch's channel shuffle ((0,2,1,3,4)),
     * the SSD head permute of an ONNX export, pixel shuffle (6-D) --, int8 / uint8 graphs: param tamd_transpose_param.  Rank 2 .. 6, the
     * order a permutation of 0 .. rank - 1 (transpose_ref.c:436-473 has one loop nest per rank and nothing for any other).  The reference
     * dequantises, moves floats and requantises EVERY element, the identity order included, so a byte of the output is one byte of the
     * input through tamd_transpose_table (int8 saturates at +-127: -128 never comes out).  fp32 graphs keep the node on the CPU device */
    /* 27: reserved, never supported (like 21 and 24: tests/test_slice_cpu.py holds the code to that answer) */
    TAMD_OP_TRANSPOSE = 28,
    /* 29: reserved, never supported (like 21, 24 and 27: tests/test_transpose_cpu.py holds the code to that answer) */
    /* the cut of RetinaFace's top-down pyramid (the x2 map of a 240 / 32 = 7.5 -> 8 row level is one row too tall for its lateral), uint8
     * graphs: param tamd_crop_param; inputs [data, like], of `like` only the shape is read.  The output has N, C, H, W of `like`
     * (crop.c:34-78) and is a box of the data's RAW bytes: ref_crop_uint8 (crop_ref.c:147-253) reads no quantisation parameter of either
     * tensor.  The caffe form (flag 0) with axis 1 (box start offset_c, offset_h, offset_w) or axis 2 (0, offset_h, offset_w) and the
     * MXNet form (flag 1) with num_args 2 (0, offset_h, offset_w).  The centre crop (num_args 1), every other flag / axis, a negative
     * offset and a box that leaves the data tensor are refused by name; int8 graphs (no kernel in the reference) and fp32 graphs keep
     * the node on the CPU device */
    TAMD_OP_CROP = 30,
    /* 31: reserved, never supported (like 21, 24, 27 and 29: tests/test_crop_cpu.py holds the code to that answer) */
    /* the not-folded BatchNorm of an MXNet / insightface export -- fc1, the last node of mobilefacenets_benchmark.tmfile --, uint8 graphs:
     * param tamd_batchnorm_param; inputs [x, gamma, beta, mean, var], the four statistics fp32 constants of C elements (caffe_flavor:
     * only mean and var are read); x 2-D [N,C], 3-D [N,C,W] or 4-D [N,C,H,W] (batchnorm_ref.c:117-141).  The reference
     * (batchnorm_kernel_ref_uint8.c:40-107) dequantises, computes x * s2[c] + s1[c] and requantises: a byte map per channel
     * (tamd_batchnorm_table), applied by chan_lut_u8 or, on large planes, by prelu_u8's per-plane form.  int8 graphs (no kernel in the
     * reference), fp32 graphs, another rank, a statistic that is no fp32 constant of C elements and a channel whose table is not
     * finite are refused by name */
    TAMD_OP_BATCHNORM = 32,
    /* 33: reserved, never supported (like 21, 24, 27, 29 and 31: tests/test_bytemap_cpu.py holds the code to that answer) */
    /* sub-pixel convolution's shuffle -- ESPCN, EDSR, torch.nn.PixelShuffle; tm2 operator 80 --, int8 / uint8 graphs: param
     * tamd_depthtospace_param.  Input (N, C, H, W), block size r >= 1 with C % (r * r) == 0; the output is (N, C / r^2, H * r, W * r)
     * (depthtospace.c infer_shape) and out[b, s, h, w] = in[b, s * r^2 + (h % r) * r + (w % r), h / r, w / r], the CRD order
     * (depthtospace_ref.c).  The reference moves RAW bytes: no quantisation parameter of either tensor is read, and the int8 byte -128
     * stays -128.  Other ranks, a block size below 1, a channel count that r^2 does not divide (the reference then silently drops
     * channels), a constant input and per-channel parameters are refused by name; fp32 graphs keep the node on the CPU device */
    TAMD_OP_DEPTHTOSPACE = 34,
    /* 35: reserved, never supported (like 21, 24, 27, 29, 31 and 33: tests/test_d2s_cpu.py holds the code to that answer) */
    /* the nearest up-sampling of an ONNX Upsample (darknet YOLOv3 / YOLOv4 exports, opset <= 9 torch exports) and caffe's Resize layer;
     * tm2 operator 54 --, int8 / uint8 graphs: param tamd_resize_param.  Input (1, C, H, W); the output is
     * (1, C, (int)(H * scale_h), (int)(W * scale_w)) (resize.c infer_shape) and output pixel (i, j) takes input pixel
     * (min((int)(i * (1.f / scale_h)), H - 1), min((int)(j * (1.f / scale_w)), W - 1)) through the byte map between the two tensors'
     * quantisation parameters (resize_ref.c:261-381; tamd_resize_indices, tamd_resize_table).  The reference defines the operator for
     * batch 1 only (its loop over the batch moves image 0 every time), and a tm2 file never carries `type`: batch > 1, bilinear (type 1),
     * other ranks, a constant input, a scale that is not finite and positive, an empty output and per-channel parameters are refused by
     * name; fp32 graphs keep the node on the CPU device */
    TAMD_OP_RESIZE = 36,
    /* 37: reserved, never supported (like 21, 24, 27, 29, 31, 33 and 35: tests/test_resize_cpu.py holds the code to that answer) */
    /* the per-image normalisation of image-to-image generators (fast style transfer, CycleGAN / pix2pix, AnimeGAN, U-Nets); tm2 operator
     * 66 --, uint8 graphs: param tamd_instancenorm_param; inputs [x, gamma, beta], x (N, C, H, W), gamma and beta fp32 constants of C
     * elements; the output has x's shape.  Per plane (n, c) the reference (instancenorm_ref.c:101-183) dequantises, sums the plane and
     * the squared deviations in two strictly sequential fp32 chains, a = gamma / sqrt(var + eps) in double, b = fma(-mean, a, beta),
     * y = fma(v, a, b), requantises: given a and b a byte map per plane (tamd_instancenorm_plane), computed ON THE DEVICE in the
     * reference's summation order (csrc/instnorm.hip).  int8 graphs (no kernel in the reference), fp32 graphs, other ranks, a constant
     * x, gamma / beta that are no finite fp32 constants of C elements, an eps that is not finite and positive, per-channel
     * parameters, an empty plane and a node whose values could leave int before the reference's conversion are refused by name */
    TAMD_OP_INSTANCENORM = 38,
    TAMD_OP_NUM
};

/* field meaning == struct conv_param (source/operator/prototype/convolution_param.h:28-45);
 * activation: -1 none, 0 relu, 1 relu1, 6 relu6 */
typedef struct tamd_conv_param {
    int kernel_h, kernel_w, stride_h, stride_w;
    int pad_h0, pad_h1, pad_w0, pad_w1;
    int dilation_h, dilation_w;
    int input_channel, output_channel, group, activation;
} tamd_conv_param;

typedef struct tamd_fc_param { int num_output; } tamd_fc_param;             /* fc_param.h */

/* == struct pool_param (pooling_param.h:34-57): pool_method 0 max / 1 avg; pads are the *original*
 * (model) pads, resolved exactly like infer_shape (pooling.c:36-100) */
typedef struct tamd_pool_param {
    int pool_method, kernel_h, kernel_w, stride_h, stride_w;
    int pad_h0, pad_h1, pad_w0, pad_w1;
    int global, caffe_flavor;
} tamd_pool_param;

typedef struct tamd_relu_param { float negative_slope; } tamd_relu_param;   /* relu_param.h */
/* field meaning == struct batchnorm_param (batchnorm_param.h) */
typedef struct tamd_batchnorm_param { float rescale_factor, eps; int caffe_flavor; } tamd_batchnorm_param;
typedef struct tamd_depthtospace_param { int block_size; } tamd_depthtospace_param;   /* depthtospace_param.h */
typedef struct tamd_instancenorm_param { float eps; } tamd_instancenorm_param;        /* instancenorm_param.h */
/* == struct resize_param (resize_param.h): type 0 nearest, 1 bilinear.  The tm2 loader fills scale_h from TM2_ResizeParam.scale_x and
 * scale_w from .scale_y and does not read .type (tm2_resize.c:42-54) */
typedef struct tamd_resize_param { float scale_w, scale_h; int type; } tamd_resize_param;
typedef struct tamd_eltwise_param { int type; int caffe_flavor; float shift, power, scale; } tamd_eltwise_param;
typedef struct tamd_concat_param { int axis; } tamd_concat_param;
typedef struct tamd_upsample_param { float scale; } tamd_upsample_param;
typedef struct tamd_permute_param { int order[4]; } tamd_permute_param;      /* permute_param.h: order0..order3 */
typedef struct tamd_softmax_param { int axis; } tamd_softmax_param;          /* softmax_param.h */
/* the RESOLVED output shape of a Reshape node (what reshape.c:37-160 infers from re_shape / is_mxnet / is_onnx); the batch
 * dimension follows tamd_graph_set_batch */
typedef struct tamd_reshape_param { int dim_num; int dims[8]; } tamd_reshape_param;
typedef struct tamd_clip_param { float max, min; } tamd_clip_param;           /* clip_param.h */
/* hardswish_param.h; carried, not used: the reference's uint8 kernel computes x * clamp(x + 3, 0, 6) / 6 whatever they hold */
typedef struct tamd_hardswish_param { float alpha, beta; } tamd_hardswish_param;
/* TM2_InterpParam order (tm2_format.h:898-905).  Both scales non-zero: the output is (int)(in * scale) per axis and the sizes are not
 * read; otherwise the sizes are, and the scales become (float)out / (float)in (interp.c:51-60) */
typedef struct tamd_interp_param { int resize_type; float width_scale, height_scale; int output_width, output_height; } tamd_interp_param;
/* split_param.h with the split_sizes vector inline.  axis: as the reference's loader leaves it (the file's value when is_onnx is set,
 * else 0).  num: the number of split_sizes; 0: the node carries none (split.c:80-117 then gives every output the input's shape);
 * -1: the is_caffe form (every output is a full copy).  The device runs num == output_num in 1 .. TAMD_SPLIT_MAX only */
#define TAMD_SPLIT_MAX 8
typedef struct tamd_split_param { int axis; int num; int sizes[TAMD_SPLIT_MAX]; } tamd_split_param;
typedef struct tamd_shufflechannel_param { int group; } tamd_shufflechannel_param;   /* shuffle_channel_param.h */
/* slice_param.h as the reference's loader and infer_shape leave it: axis normalised into [0, rank) (slice.c:52-53), begin / end / step of
 * the onnx and mxnet forms (a stored step of 0 means 1), the three form flags.  The three vectors of the caffe and tf forms are not
 * carried, only their element counts, so that those forms can be refused by name */
typedef struct tamd_slice_param {
    int axis, begin, end, step;
    int iscaffe, ismxnet, isonnx;
    int slice_point_num, begin_num, size_num;
} tamd_slice_param;
/* transpose_param.h: the tr_shape vector inline.  dim_num: its length as the file stores it (any value: a length the device does not
 * run is refused by name; only the first 8 entries are carried); out.dims[i] = in.dims[order[i]] (transpose.c:35-54) */
typedef struct tamd_transpose_param { int dim_num; int order[8]; } tamd_transpose_param;
/* crop_param.h, field for field */
typedef struct tamd_crop_param { int num_args, offset_c, offset_h, offset_w, crop_h, crop_w, center_crop, axis, flag; } tamd_crop_param;

/* == struct priorbox_param (source/operator/prototype/priorbox_param.h:28-52) with the float vectors inline; num_priors /
 * out_dim are re-derived as priorbox.c:37-64 does.  inputs: [0] feature map, [1] the image ("data") -- shapes only */
#define TAMD_PRIORBOX_MAX 8
typedef struct tamd_priorbox_param {
    int min_size_num, max_size_num, aspect_ratio_num;
    float min_size[TAMD_PRIORBOX_MAX], max_size[TAMD_PRIORBOX_MAX], aspect_ratio[TAMD_PRIORBOX_MAX], variance[4];
    int flip, clip, image_h, image_w;
    float step_h, step_w, offset;
} tamd_priorbox_param;

/* == the quantisation-relevant part of struct tensor (source/graph/tensor.h:43-102) */
typedef struct tamd_tensor_desc {
    int dtype;            /* TAMD_DT_*                                            */
    int ttype;            /* TAMD_TT_*                                            */
    int dim_num;
    int dims[8];          /* NCHW / OIHW / [out][hidden] / [n]                    */
    const void* data;     /* const payload (host, copied at prerun), else NULL    */
    int quant_num;        /* 0 none, 1 per-tensor, N per-channel                  */
    const float* scales;  /* quant_num entries                                    */
    const int* zero_points;
    const char* name;     /* optional                                             */
} tamd_tensor_desc;

typedef struct tamd_node_desc {
    int op;               /* TAMD_OP_*                                            */
    int input_num;
    const int* inputs;    /* tensor indices                                       */
    int output_num;
    const int* outputs;
    const void* param;    /* op specific struct above, or NULL                    */
    const char* name;
} tamd_node_desc;

/* == the device option blob passed through set_context_device (first field is dev_name by the
 * reference's convention, trt_define.h:35-41 / scheduler.c:49-57) */
typedef struct tamd_options {
    const char* dev_name; /* "HIP"                                                */
    int size;             /* sizeof(tamd_options) as the CALLER compiled it: set_context_device copies dev_opt_size bytes
                           * and hands pre_run only the pointer (c_api.c:183-210, scheduler.c:49-57), so the blob
                           * carries its own size; fields beyond it keep their defaults (0: only dev_name is read) */
    int gpu_index;        /* HIP device ordinal                                   */
    int use_hip_graph;    /* 1: capture the launch list into a hipGraph (default) */
    int profile;          /* 1: print a per-launch timing table on stderr when the graph is released -- what
                           * TG_DEBUG_TIME=1 makes the CPU device do (cpu_define.h:41-43, cpu_dump.c:607-697); the
                           * environment variable itself is honoured too */
    int direct_dispatch;  /* 1: tamd_graph_launch replays the launch list as AQL packets on the graph's own HSA queue instead
                           * of hipGraphLaunch (shorter launch boundaries, no hole between replays; csrc/direct.cc).  The
                           * passes queued between two calls that wait (tamd_graph_sync / _download_outputs / _upload_inputs /
                           * _run / _read_tensor ...) all compute the same input and are observed TOGETHER by the next such call;
                           * a graph with two slots (split_batch below, tamd_graph_slots) runs two of them at a time on two HSA
                           * queues, so they are not ordered among themselves -- nothing a caller can see depends on that order.
                           * Work on tamd_graph_stream() is NOT ordered behind them.  TAMD_DIRECT_DISPATCH=0|1
                           * overrides.  Falls back to the hipGraph silently when the list cannot be dispatched directly. */
    int keep_tensors;     /* 1: every intermediate tensor keeps a buffer of its own, so tamd_graph_read_tensor can return any of
                           * them after a run (the TG_DEBUG_DATA analogue).  0 (default): tensors whose lifetimes do not overlap
                           * share device memory -- a pass then touches a fraction of the bytes, which is what keeps the batched
                           * configs inside the device's last-level cache; read_tensor refuses such tensors.  TAMD_POOL=0|1
                           * overrides (0 = keep). */
    int u8_integer;       /* 1: uint8 convolutions (group 1) run as EXACT int32 sums on the int8 matrix cores and are requantised
                           * once -- every CONVOLUTION is within ONE quantisation step of the reference CPU backend on the reference's
                           * own inputs (teacher-forced, tests/test_gpu_u8_int.py), not byte-identical (the reference simulates uint8
                           * in fp32, conv_kernel_x86.c:68-80,1703-1794).  The bound is per layer, NOT end to end: errors compound,
                           * MobileNet-SSD's outputs differ from the reference's by up to 4-5 steps in 33-36 % of the bytes
                           * (profiles/r04_u8int_pytest.txt).  0 (default): the byte-exact fp32 chains.  TAMD_U8_INT=0|1 overrides. */
    int split_batch;      /* A batched graph whose operators treat the images of a batch independently (Convolution, FullyConnected,
                           * Pooling, ReLU, Eltwise, Dropout, Sigmoid, Clip, HardSwish, Mish, Concat / Softmax on an axis >= 1) and whose activation tensors all carry
                           * the same even batch B as dimension 0 can be compiled as TWO device graphs of B / 2 images each, run side by
                           * side on their own HSA queues behind this one tamd_graph: launch boundaries and tile tails of one half
                           * overlap the other half's work (ResNet-50 b32 +8 %, MobileNet-v1 b64 +6 %, outputs identical:
                           * profiles/r06_split_batch_direct.txt).  Every entry point behaves as for one graph; host buffers are used
                           * as two contiguous halves.  0 (default): where it pays -- int8 graphs with direct_dispatch from batch 16
                           * on; 1: never (final: a caller that splits batches by itself, as the plugin does); 2: wherever it is possible.
                           * TAMD_SPLIT_BATCH=0|1|2 overrides 0 and 2 (0: never, 1: default rule, 2: wherever possible -- the values the
                           * plugin's switch of the same name takes).  tamd_graph_halves() tells which form a graph took.
                           *   TWO SLOTS (csrc/graph_slots.hip): a graph that is not such a pair may instead keep two passes of its ONE
                           * launch list in flight -- a second program of the list on a second HSA queue, with everything a pass writes
                           * re-pointed at a private copy (weights, tables and the input staging buffers are shared), and
                           * tamd_graph_launch alternating between the two.  This raises THROUGHPUT where a pass leaves the device idle
                           * (int8 MobileNet-v1 batch 1: 27.7 us per pass against 49.2, profiles/two_slots_ab.txt); it does not shorten
                           * a pass: tamd_graph_run, a lone launch + sync and tamd_graph_time_launches are what they were.  0 (default):
                           * int8 graphs with direct_dispatch at batch 1; 1: never; 2: every int8 graph with direct_dispatch that is
                           * not a pair.  A list that does not qualify (a launch that ran once at prerun, no second queue, a slot that
                           * does not reproduce the eager pass byte for byte at prerun) stays one list, silently (TAMD_DEBUG=1 says
                           * why).  tamd_graph_slots() tells. */
} tamd_options;
/* does a blob that carries `size` hold `field` whole?  Every reader of a caller's blob asks this field by field; a field the blob
 * does not reach keeps the reader's default */
#define TAMD_OPTIONS_HAS(size, field) ((size) >= (int)(offsetof(tamd_options, field) + sizeof(((const tamd_options*)0)->field)))

typedef struct tamd_graph tamd_graph;

/* ---- device: what struct interface.init / release_device and allocator.describe need
 * (source/device/device.h:40-84; the CUDA backend's equivalents: cuda_device.cc:47-83,212-238) ---- */
TAMD_API int tamd_device_count(void);
TAMD_API int tamd_init(int gpu_index);
TAMD_API int tamd_shutdown(void);
TAMD_API const char* tamd_last_error(void);
TAMD_API const char* tamd_version(void);
/* 1 if (op, dtype) can run on the device -- what allocator.describe publishes */
TAMD_API int tamd_op_supported(int op, int dtype);
/* 1 if this node with these parameters and tensors (descriptors only; the one const payload read, where it is given, is a PReLU's
 * slope: a value that widens to inf or NaN is refused; a Slice and a Transpose need the scales and zero points of both tensors, for their byte maps) is one the device
 * compiles; 0 -> leave it to the CPU device.  Replaces the per-op parameter tests a backend makes while it walks a
 * subgraph (source/device/cuda/cuda_executor.cc:72-134 fails Build() instead; tensorrt: trt_limit.hpp) */
TAMD_API int tamd_node_supported(const tamd_node_desc* node, const tamd_tensor_desc* inputs, int input_num,
                                 const tamd_tensor_desc* outputs, int output_num);
/* the byte map the device applies for a Sigmoid / Clip / HardSwish / Mish node between tensors of these quantisation parameters:
 * table[b] = the output byte for input byte b (int8: b is the byte's bit pattern).  param: the operator's struct above (NULL where it
 * has none).  Built on the host with the reference's own float / double arithmetic; needs no GPU.  0, or -1 for an (op, dtype) pair
 * the device does not run */
TAMD_API int tamd_lut_table(int op, int dtype, const void* param, float in_scale, int in_zp, float out_scale, int out_zp,
                            unsigned char table[256]);
/* the byte maps of an Eltwise node with a constant one-element second operand, or with no second operand (csrc/lut_tables.cc; no GPU
 * needed), dtype TAMD_DT_INT8 | TAMD_DT_UINT8 (eltwise_ref.c:589-847 | :311-587).
 * tamd_eltwise_table: table[raw input byte] = the raw output byte: the byte dequantised (uint8 (u - zero) * scale, int8 (float)q * scale),
 * the operator's line against `scalar` (the types that read one: PROD 0, PROD_SCALAR 1, SUM 2, SUB 4, SUB_SCALAR 5, MIN_SCALAR 8,
 * DIV 10) or alone (RSQRT 7, LOG 11, EXP 12, SQRT 13, FLOOR 14, SQUARE 15, POWER 17: pow(shift + scale * x, power) of `param`, which the
 * other types do not read), round(f / out_scale) (+ out_zp) clamped to -127 .. 127 | 0 .. 255.  0; -1 for another type or dtype (or
 * POWER without param); -2 when one of the 256 values before the clamp is NaN, infinite or outside int -- RSQRT or LOG of a tensor whose
 * zero-point byte is 0.0, a division by 0: the reference's conversion is undefined there and the node is refused.
 * tamd_eltwise_scalar: the float the kernels make of the constant's first element: an fp32 constant as it is (uint8 graphs only), a
 * uint8 one (u - zp) * scale, an int8 one (float)q * scale.  0, or -1 for another type.
 * tamd_eltwise_pair: the output byte (0 .. 255, int8 as its bit pattern) of the same-shape PROD 0 / SUM 2 / SUB 4 / MAX 6 on ONE pair of
 * bytes; -1 for another type or dtype, -2 where the conversion is undefined */
TAMD_API int tamd_eltwise_table(int type, int dtype, const tamd_eltwise_param* param, float scalar, float in_scale, int in_zp,
                                float out_scale, int out_zp, unsigned char table[256]);
TAMD_API int tamd_eltwise_scalar(int const_dtype, const void* value, float scale, int zp, float* scalar);
TAMD_API int tamd_eltwise_pair(int type, int dtype, unsigned char a, float a_scale, int a_zp, unsigned char b, float b_scale, int b_zp,
                               float out_scale, int out_zp);
/* the byte map of ONE channel of a uint8 BatchNorm (csrc/lut_tables.cc; no GPU needed), batchnorm_ref.c:76-86 and
 * batchnorm_kernel_ref_uint8.c:57-101 as the built reference's compiler contracts them: rescale = rescale_factor ? 1 / rescale_factor : 0;
 * scale_var_inv = 1 / sqrtf(fmaf(var, rescale, eps)); scale_mean = -mean * (rescale * scale_var_inv); s1 = scale_mean, s2 =
 * scale_var_inv, unless caffe_flavor: s1 = fmaf(gamma, scale_mean, beta), s2 = gamma * scale_var_inv; table[b] = (int)roundf(fmaf(((float)b
 * - (float)in_zp) * in_scale, s2, s1) / out_scale + (float)out_zp) clamped to 0 .. 255.  0; -1 without param or table; -2 when s1, s2 or
 * one of the 256 values before the clamp is not finite or lies outside int (the node is refused) */
TAMD_API int tamd_batchnorm_table(const tamd_batchnorm_param* param, float gamma, float beta, float mean, float var, float in_scale, int in_zp,
                                  float out_scale, int out_zp, unsigned char table[256]);
/* ONE plane of a uint8 InstanceNorm (csrc/instnorm_tables.cc; no GPU needed): the specification of the device kernels, every operation
 * as the built reference's object code has it.  x[0 .. size): the plane's bytes.  v_j = ((float)x_j - (float)in_zp) * in_scale;
 * sum = the sequential fp32 sum over j ascending; mean = sum / size; sqsum over j ascending of t = v_j - mean: sqsum + t * t with the
 * product ROUNDED for j < size - size % 4 and fmaf(t, t, sqsum) for the last size % 4 elements; var = sqsum / size;
 * a = (float)((double)gamma / sqrt((double)(var + eps))); b = fmaf(-mean, a, beta); table[u] = (int)roundf(fmaf(v(u), a, b) / out_scale +
 * (float)out_zp) clamped to 0 .. 255.  stats (may be null): {sum, sqsum, a, b}.  0; -1: bad arguments (size < 1); -2: a table value is NaN or
 * outside int */
TAMD_API int tamd_instancenorm_plane(const unsigned char* x, int size, float gamma, float beta, float eps, float in_scale, int in_zp, float out_scale,
                                     int out_zp, unsigned char table[256], float stats[4]);
/* the two host-built operands of a nearest Interp node (csrc/interp_tables.cc; no GPU needed).
 * tamd_interp_table: table[b] = the output byte for input byte b between tensors of these quantisation parameters (interp_ref.c:269-272,
 * 346-354: int8 saturates at +-127, so -128 comes out as -127 even between equal scales; :378-381, 455-463: uint8 at 0 .. 255).  0, or
 * -1 for a dtype other than int8 / uint8.
 * tamd_interp_indices: idx[o] = (int)((float)o / scale) for o in [0, out_extent), the source row / column of output row / column o
 * (interp_ref.c:292-293).  0, or -1 when an index leaves [0, in_extent) -- the reference would read out of bounds there -- or an
 * extent is not positive */
TAMD_API int tamd_interp_table(int dtype, float in_scale, int in_zp, float out_scale, int out_zp, unsigned char table[256]);
TAMD_API int tamd_interp_indices(int in_extent, int out_extent, float scale, int* idx);
/* the two host-built operands of a nearest Resize node (csrc/resize_tables.cc; no GPU needed).
 * tamd_resize_table: table[b] = the output byte for input byte b between tensors of these quantisation parameters (resize_ref.c:288,
 * :310-315: int8 saturates at +-127, so -128 comes out as -127 even between equal parameters; :349, :371-376: uint8 at 0 .. 255) -- the
 * lines of tamd_interp_table, and its implementation.  0; -1 for a dtype other than int8 / uint8; -2 when one of the 256 values before
 * its conversion to int is not finite or lies outside int: the reference's conversion is undefined there and the node is refused.
 * tamd_resize_indices: idx[o] = min((int)((float)o * (1.f / scale)), in_extent - 1) for o in [0, out_extent), the source row / column
 * of output row / column o (resize_ref.c:298, :301, :409-410); `scale` is the node's own scale_h / scale_w, the reciprocal is formed
 * here.  0, or -1 when the scale is not finite and positive, an extent is not positive or a product leaves int */
TAMD_API int tamd_resize_table(int dtype, float in_scale, int in_zp, float out_scale, int out_zp, unsigned char table[256]);
TAMD_API int tamd_resize_indices(int in_extent, int out_extent, float scale, int* idx);
/* the two host-built operands of the channel-moving operators (csrc/chanmap_tables.cc; no GPU needed).
 * tamd_shuffle_sources: src[o] = the input channel that output channel o of a ShuffleChannel node takes: src[group * j + i] =
 * (channels / group) * i + j (shuffle_channel_ref.c).  0, or -1 for group < 1 or channels % group != 0 -- the reference never writes the
 * last channels then.
 * tamd_split_table: table[b] = the output byte of a uint8 Split for input byte b (split_ref.c:94-99, as the compiler contracts it:
 * roundf(fmaf((float)(b - in_zp), in_scale / out_scale, (float)out_zp)) clamped to 0 .. 255).  An int8 Split copies bytes and has no
 * table.  0, or -1 without a table */
TAMD_API int tamd_shuffle_sources(int channels, int group, int* src);
TAMD_API int tamd_split_table(float in_scale, int in_zp, float out_scale, int out_zp, unsigned char table[256]);
/* the byte map of a uint8 Slice between tensors of these quantisation parameters (csrc/slice_tables.cc; no GPU needed): table[b] =
 * round(((float)b - (float)in_zp) * in_scale / out_scale + (float)out_zp) clamped to 0 .. 255 -- every step a float operation of its own,
 * the rounding the double round() (slice_ref.c:488-505).  0, or -1 when a scale is not finite and positive or one of the 256 values
 * before the clamp is not finite or lies outside int: the reference's conversion is undefined there and the node is refused */
TAMD_API int tamd_slice_table(float in_scale, int in_zp, float out_scale, int out_zp, unsigned char table[256]);
/* the byte map of a Transpose between tensors of these quantisation parameters (csrc/transpose_tables.cc; no GPU needed), dtype
 * TAMD_DT_INT8 | TAMD_DT_UINT8: table[raw input byte] = the raw output byte (int8 in two's complement) --
 * round(((float)q - (float)in_zp) * in_scale / out_scale + (float)out_zp), every step a float operation of its own, the rounding the
 * double round(), clamped to -127 .. 127 | 0 .. 255 (transpose_ref.c:290, :317-322 | :348, :375-380).  0, or -1 for another dtype and
 * when one of the 256 values before the clamp is not finite or lies outside int: the reference's conversion is undefined there and
 * the node is refused */
TAMD_API int tamd_transpose_table(int dtype, float in_scale, int in_zp, float out_scale, int out_zp, unsigned char table[256]);
/* the host truth of a quantised PReLU node (csrc/prelu_tables.cc; no GPU needed).
 * tamd_prelu_slope: the float the reference makes of one fp16 slope (bit pattern), as its fp16_to_fp32 (source/utility/float.c) does
 * on x86: normal halves with a non-zero fraction and infinities as IEEE; a normal half whose fraction is zero -- every exact power of
 * two -- gives +0.0f; a sub-normal half gets its fraction in the low bits of the field (0x0003 -> 0x34000200); NaN gets fraction 1.
 * tamd_prelu_table: table[b] = the output byte of one channel for input byte b (int8: b is the byte's bit pattern) with this slope
 * between tensors of these quantisation parameters: MAX(x, 0) + slope * MIN(x, 0) in float, round(y / scale [+ zero]) saturated to
 * +-127 (int8: -128 never comes out) or 0 .. 255 (uint8).  0, or -1 for a dtype other than int8 / uint8 and for a slope that widens
 * to inf or NaN */
TAMD_API float tamd_prelu_slope(unsigned short half_bits);
TAMD_API int tamd_prelu_table(int dtype, unsigned short slope_bits, float in_scale, int in_zp, float out_scale, int out_zp,
                              unsigned char table[256]);

/* ---- graph construction: the plugin's pre_run walks `struct subgraph` (source/graph/subgraph.h, node.h:46-70,
 * tensor.h:43-102) and mirrors it through these calls, like CUDAEngine::Build does for its own IR
 * (source/device/cuda/cuda_executor.cc:72-134) ------------------------------------------------- */
TAMD_API tamd_graph* tamd_graph_create(void);
TAMD_API int tamd_graph_add_tensor(tamd_graph* g, const tamd_tensor_desc* desc);  /* -> tensor index or <0 */
TAMD_API int tamd_graph_add_node(tamd_graph* g, const tamd_node_desc* desc);      /* -> node index or <0   */
TAMD_API int tamd_graph_set_inputs(tamd_graph* g, int n, const int* tensor_ids);
TAMD_API int tamd_graph_set_outputs(tamd_graph* g, int n, const int* tensor_ids);
/* parse tmfile-v2 bytes (the reference's own model format); the buffer may be freed afterwards */
TAMD_API tamd_graph* tamd_graph_load_tm2(const void* mem, size_t size);
/* re-shape the batch dimension of every input (== set_tensor_shape + infer_shape) before prerun */
TAMD_API int tamd_graph_set_batch(tamd_graph* g, int batch);

/* ---- execution ----------------------------------------------------------------------------
 * Threading: the library may be used from several host threads, each graph by ONE thread at a time (a graph's run state --
 * I/O slots, runs in flight, its HSA queue, which is single-producer -- is not locked; the reference calls a subgraph's
 * interface from one scheduler thread as well, scheduler.c:95-213).  Different graphs never share run state.
 * Enforced since round 5: a call that arrives while ANOTHER thread is inside a call on the same graph returns -1
 * ("... one graph = one thread at a time"); calls from different threads one after the other are fine.
 * prerun  <- interface.pre_run   (device.h:46, called from scheduler.c:49-59; options may be NULL)
 * run     <- interface.run       (device.h:49, scheduler.c:134; must return with outputs complete)
 * destroy <- interface.post_run / release_graph (device.h:52-58, scheduler.c:201, subgraph.c:53-56) */
TAMD_API int tamd_graph_prerun(tamd_graph* g, const tamd_options* opt);
/* 2: the graph was compiled as two half-batch device graphs (tamd_options.split_batch); 0: one launch list */
TAMD_API int tamd_graph_halves(const tamd_graph* g);
/* 2: tamd_graph_launch keeps two passes of the launch list in flight on two HSA queues (tamd_options.split_batch, "two slots");
 * 0: one pass at a time.  Every other entry point behaves alike in both forms. */
TAMD_API int tamd_graph_slots(const tamd_graph* g);
TAMD_API int tamd_graph_input_num(const tamd_graph* g);
TAMD_API int tamd_graph_output_num(const tamd_graph* g);
/* dims/dtype of graph input / output `idx` (NCHW); returns dim_num */
TAMD_API int tamd_graph_input_desc(const tamd_graph* g, int idx, int* dims8, int* dtype);
TAMD_API int tamd_graph_output_desc(const tamd_graph* g, int idx, int* dims8, int* dtype, float* scale, int* zero_point);
/* host NCHW buffers; the input pointer is re-read at every run (tm_benchmark.cc:95-102 semantics) */
TAMD_API int tamd_graph_set_input(tamd_graph* g, int idx, const void* host_nchw, size_t bytes);
TAMD_API int tamd_graph_set_output(tamd_graph* g, int idx, void* host_nchw, size_t bytes);
/* H2D inputs -> kernels -> D2H outputs; returns when outputs are complete (scheduler is synchronous) */
TAMD_API int tamd_graph_run(tamd_graph* g);
/* asynchronous pair <- interface.async_run / async_wait (device.h:60-63; the reference's scheduler never issues them:
 * run_graph(graph, 0) is rejected, scheduler.c:75-79).  run_async stages the current input buffers, queues H2D -> kernels ->
 * D2H and returns; up to TWO runs may be in flight (a third submit fails); wait blocks for the OLDEST one and delivers its
 * outputs to the buffers that were set when it was submitted.  Same bytes as tamd_graph_run; with direct dispatch each run is one
 * burst on the graph's HSA queue (the second queues behind the first's closing packet), else both ride the graph's stream.
 * While runs are in flight the other entry points that touch the I/O buffers (run, upload_inputs, download_outputs) fail. */
TAMD_API int tamd_graph_run_async(tamd_graph* g);
TAMD_API int tamd_graph_wait(tamd_graph* g);
TAMD_API int tamd_graph_inflight(const tamd_graph* g);   /* runs submitted and not yet waited for */
/* HBM-resident variants (measurement, multi-GPU harness): stage inputs once, launch without copies */
TAMD_API int tamd_graph_upload_inputs(tamd_graph* g);
TAMD_API int tamd_graph_launch(tamd_graph* g);            /* async on the graph's stream          */
TAMD_API int tamd_graph_sync(tamd_graph* g);
/* packets per pass when tamd_graph_launch dispatches directly (tamd_options.direct_dispatch took effect), else 0 */
TAMD_API int tamd_graph_direct_packets(const tamd_graph* g);
/* of those packets, how many carry hidden arguments placed at the offsets the kernel's own code-object metadata lists (the rest
 * use the code-object-v5 default layout, vouched for by the prerun self-check) */
TAMD_API int tamd_graph_direct_meta_packets(const tamd_graph* g);
/* MEASUREMENT (round 6): `passes` back-to-back passes of the directly dispatched launch list with every packet stamped by the HSA
 * runtime's own dispatch profiling (hsa_amd_profiling_get_dispatch_time -- the timestamps a kernel trace reports, without a tool
 * intercepting the queue): dur_us[i] = mean duration of packet i, gap_us[i] = mean time from its end to the next packet's start
 * (the last packet: to the first packet of the next pass).  On this stack the stamps of consecutive barrier-bit packets ABUT (gap 0): a
 * packet's "duration" is its kernel plus the launch boundary in front of it, and the per-packet completion signals the stamps need cost
 * ~0.6 us per packet -- the sums equal the host's clock of an unstamped pass within 0.5 % on the batched configs, +18 % at batch 1.  Returns the packet count (<= max_packets), -1 when the graph does not
 * dispatch directly.  tamd_graph_direct_packet_name(g, i): kernel symbol of packet i. */
TAMD_API int tamd_graph_direct_timestamps(tamd_graph* g, int passes, double* dur_us, double* gap_us, int max_packets);
TAMD_API const char* tamd_graph_direct_packet_name(const tamd_graph* g, int i);
/* MEASUREMENT, a graph with two slots: ONE burst of `passes` rounds, each a pass on slot 0's queue and a pass on slot 1's, every
 * packet stamped as above.  Raw stamps in microseconds on the common clock, counted from the earliest start:
 * start_us / end_us[(round * 2 + slot) * packets + packet], packets = tamd_graph_direct_packets().  Returns the rounds stamped
 * (max_stamps >= passes * 2 * packets), -1 when the graph has one slot.  tamd_graph_direct_timestamps and tamd_graph_time_launches keep
 * running slot 0 ALONE: they describe a pass as the dependent chain it is. */
TAMD_API int tamd_graph_slot_timestamps(tamd_graph* g, int passes, double* start_us, double* end_us, int max_stamps);
TAMD_API int tamd_graph_download_outputs(tamd_graph* g);
/* device pointer + byte size of graph output `idx` in the reference's NCHW order (for RCCL gather).  Valid after any pass: a
 * direct-dispatch tamd_graph_run / tamd_graph_wait leaves its outputs in the pinned host buffers only (zero-copy lists) and this
 * call refreshes the device copy from there first; it fails while asynchronous runs are in flight.  For a graph compiled as two
 * half-batch device graphs (tamd_options.split_batch) the pointer is a buffer of the pair into which THIS CALL gathers the two halves'
 * outputs (it waits for their passes first): call it after the pass whose outputs are wanted, not once before a loop of passes.
 * With two slots (tamd_graph_slots) the pointer stays what it is for one list: a PERSISTENT view of slot 0's buffer, taken once,
 * valid after every tamd_graph_sync, no copy -- slot 0 runs first after every call that waits, and every pass since computed the same
 * bytes. */
TAMD_API int tamd_graph_output_device(tamd_graph* g, int idx, void** dptr, size_t* bytes);
TAMD_API void* tamd_graph_stream(tamd_graph* g);          /* hipStream_t                           */
/* wall time tamd_graph_prerun took (planning incl. the plan-time autotune, capture, direct-dispatch programs), milliseconds */
TAMD_API double tamd_graph_prerun_ms(const tamd_graph* g);
/* time `iters` back-to-back launches with HIP events on the graph's stream -> total ms (direct dispatch: the host's clock around
 * submit .. complete, on ONE queue -- slot 0 alone where the graph has two slots: the duration of a pass, not the throughput step) */
TAMD_API int tamd_graph_time_launches(tamd_graph* g, int iters, float* total_ms);

/* ---- introspection / profiling: the TG_DEBUG_TIME / TG_DEBUG_DATA analogues of the CPU device
 * (source/device/cpu/cpu_define.h:41-43, cpu_dump.c:607-697) ---------------------------------- */
typedef struct tamd_kernel_info {
    char node[64];        /* graph node name                                     */
    char kernel[48];      /* device kernel family                                */
    double macs;          /* multiply-accumulates of this launch                 */
    double bytes;         /* algorithmic bytes: in + out + weights (+bias)       */
    float ms;             /* average duration (tamd_graph_profile)               */
} tamd_kernel_info;
TAMD_API int tamd_graph_kernel_num(const tamd_graph* g);
/* eager per-launch timing with hipEvent pairs on the graph's stream, averaged over `iters` */
TAMD_API int tamd_graph_profile(tamd_graph* g, int iters, tamd_kernel_info* out, int max_out);
/* copy any tensor back to host in NCHW (debug / layer-by-layer parity, cf. TG_DEBUG_DATA) */
TAMD_API int tamd_graph_read_tensor(tamd_graph* g, int tensor_idx, void* host_nchw, size_t bytes);
TAMD_API int tamd_graph_tensor_num(const tamd_graph* g);
TAMD_API int tamd_graph_tensor_desc(const tamd_graph* g, int tensor_idx, int* dims8, int* dtype);
/* the byte-pure chain that starts at table node `node` (index in the order the nodes were added) of a loaded int8 / uint8 graph, as the
 * planners look for it before their own layout conditions: table nodes (Sigmoid / Clip / HardSwish / Mish, scalar and unary Eltwise)
 * and same-shape Eltwise nodes whose output byte is a function of ONE byte of the first node's input, none of whose intermediate
 * tensors has a reader outside the chain or is a graph output.  Such a chain runs as one lut_u8 launch.  nodes[0 .. min(count, cap)): the
 * members in node order; table[b]: the byte of the last member's output where the source holds byte b -- every node evaluated with
 * the reference's arithmetic (tamd_lut_table, tamd_eltwise_table, tamd_eltwise_pair).  The member count (>= 2); 0: no chain starts
 * there (or TAMD_PIN=bytemap_chain=0); -1: bad arguments.  Needs no GPU and no prerun */
TAMD_API int tamd_graph_bytemap_chain(const tamd_graph* g, int node, int* nodes, int cap, unsigned char table[256]);
/* how the uint8 planner runs InstanceNorm node `node` (index in the order the nodes were added) of a loaded graph: *form 0: instnorm_stats_u8
 * writes the planes' byte maps, chan_lut_u8 applies them (two launches; the default on planes above 4096 bytes); 1: instnorm_u8 does both (one
 * launch; the default up to 4096 bytes a plane; TAMD_PIN=instnorm_form forces either).
 * *relu_node: the index of the ReLU / leaky ReLU composed into the map -- the output's only reader, the output no graph output,
 * TAMD_PIN=instnorm_relu=0 not set --, -1: none.  Asked before buffers are planned, this is an UPPER BOUND: prerun keeps a ReLU a launch
 * of its own where its output turns out to be written in place into a Concat's buffer, or where another launch has taken the node.  0; -1: bad arguments or no InstanceNorm node the device runs.  Needs no GPU and no prerun */
TAMD_API int tamd_graph_instancenorm_plan(const tamd_graph* g, int node, int* form, int* relu_node);

TAMD_API void tamd_graph_destroy(tamd_graph* g);

#ifdef __cplusplus
}
#endif
#endif
