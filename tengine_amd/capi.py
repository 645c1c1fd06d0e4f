"""ctypes binding of the C ABI (include/tengine_amd.h) -- the only way Python reaches the device.

There is NO CPU fallback: if the native library is missing, or no HIP device is visible at prerun,
the calls raise (the CPU oracle lives in oracle/ and is test infrastructure only).
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libtengine_amd.so")

DT_FP32, DT_FP16, DT_INT8, DT_UINT8, DT_INT32 = 0, 1, 2, 3, 4
_NP = {DT_FP32: np.float32, DT_FP16: np.float16, DT_INT8: np.int8, DT_UINT8: np.uint8, DT_INT32: np.int32}


class Options(C.Structure):           # tamd_options
    _fields_ = [("dev_name", C.c_char_p), ("size", C.c_int), ("gpu_index", C.c_int), ("use_hip_graph", C.c_int), ("profile", C.c_int),
                ("direct_dispatch", C.c_int), ("keep_tensors", C.c_int), ("u8_integer", C.c_int), ("split_batch", C.c_int)]


class KernelInfo(C.Structure):        # tamd_kernel_info
    _fields_ = [("node", C.c_char * 64), ("kernel", C.c_char * 48), ("macs", C.c_double), ("bytes", C.c_double),
                ("ms", C.c_float)]


EXPORTS = [
    "tamd_device_count", "tamd_init", "tamd_shutdown", "tamd_last_error", "tamd_version", "tamd_op_supported", "tamd_node_supported", "tamd_lut_table", "tamd_eltwise_table", "tamd_eltwise_scalar", "tamd_eltwise_pair", "tamd_batchnorm_table", "tamd_instancenorm_plane", "tamd_interp_table", "tamd_interp_indices", "tamd_resize_table", "tamd_resize_indices", "tamd_shuffle_sources", "tamd_split_table", "tamd_slice_table", "tamd_transpose_table", "tamd_prelu_slope", "tamd_prelu_table",
    "tamd_graph_create", "tamd_graph_add_tensor", "tamd_graph_add_node", "tamd_graph_set_inputs",
    "tamd_graph_set_outputs", "tamd_graph_load_tm2", "tamd_graph_set_batch", "tamd_graph_prerun", "tamd_graph_halves", "tamd_graph_slots",
    "tamd_graph_input_num", "tamd_graph_output_num", "tamd_graph_input_desc", "tamd_graph_output_desc",
    "tamd_graph_set_input", "tamd_graph_set_output", "tamd_graph_run", "tamd_graph_run_async", "tamd_graph_wait", "tamd_graph_inflight", "tamd_graph_upload_inputs",
    "tamd_graph_launch", "tamd_graph_sync", "tamd_graph_direct_packets", "tamd_graph_direct_meta_packets", "tamd_graph_download_outputs", "tamd_graph_output_device",
    "tamd_graph_direct_timestamps", "tamd_graph_slot_timestamps", "tamd_graph_direct_packet_name", "tamd_graph_stream", "tamd_graph_time_launches", "tamd_graph_prerun_ms", "tamd_graph_kernel_num", "tamd_graph_profile",
    "tamd_graph_read_tensor", "tamd_graph_tensor_num", "tamd_graph_tensor_desc", "tamd_graph_bytemap_chain", "tamd_graph_instancenorm_plan", "tamd_graph_destroy",
]

_lib = None


class TamdError(RuntimeError):
    pass


def version():
    return lib().tamd_version().decode()


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TamdError("native library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(tengine_amd has no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp, ci = C.c_void_p, C.c_int
        L.tamd_last_error.restype = C.c_char_p
        L.tamd_version.restype = C.c_char_p
        L.tamd_graph_create.restype = vp
        L.tamd_graph_load_tm2.restype = vp
        L.tamd_graph_load_tm2.argtypes = [vp, C.c_size_t]
        L.tamd_graph_stream.restype = vp
        L.tamd_graph_direct_packet_name.restype = C.c_char_p
        L.tamd_graph_direct_packet_name.argtypes = [vp, ci]
        L.tamd_graph_direct_timestamps.argtypes = [vp, ci, C.POINTER(C.c_double), C.POINTER(C.c_double), ci]
        # (guarded: tools/exp/ab_lib.py loads an OLDER build of the library under this binding, which has no slots)
        if hasattr(L, "tamd_graph_slots"):
            L.tamd_graph_slot_timestamps.argtypes = [vp, ci, C.POINTER(C.c_double), C.POINTER(C.c_double), ci]
            L.tamd_graph_slots.argtypes = [vp]
        L.tamd_graph_prerun_ms.restype = C.c_double
        L.tamd_graph_prerun_ms.argtypes = [vp]
        for name, args in {
            "tamd_graph_set_batch": [vp, ci], "tamd_graph_prerun": [vp, C.POINTER(Options)],
            "tamd_graph_input_num": [vp], "tamd_graph_output_num": [vp], "tamd_graph_halves": [vp],
            "tamd_graph_input_desc": [vp, ci, C.POINTER(ci), C.POINTER(ci)],
            "tamd_graph_output_desc": [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_float), C.POINTER(ci)],
            "tamd_graph_set_input": [vp, ci, vp, C.c_size_t], "tamd_graph_set_output": [vp, ci, vp, C.c_size_t],
            "tamd_graph_run": [vp], "tamd_graph_run_async": [vp], "tamd_graph_wait": [vp], "tamd_graph_inflight": [vp],
            "tamd_graph_upload_inputs": [vp], "tamd_graph_launch": [vp],
            "tamd_graph_sync": [vp], "tamd_graph_direct_packets": [vp], "tamd_graph_direct_meta_packets": [vp], "tamd_graph_download_outputs": [vp],
            "tamd_graph_output_device": [vp, ci, C.POINTER(vp), C.POINTER(C.c_size_t)],
            "tamd_graph_stream": [vp], "tamd_graph_time_launches": [vp, ci, C.POINTER(C.c_float)],
            "tamd_graph_kernel_num": [vp], "tamd_graph_profile": [vp, ci, C.POINTER(KernelInfo), ci],
            "tamd_graph_read_tensor": [vp, ci, vp, C.c_size_t], "tamd_graph_tensor_num": [vp],
            "tamd_graph_tensor_desc": [vp, ci, C.POINTER(ci), C.POINTER(ci)], "tamd_graph_destroy": [vp],
            "tamd_init": [ci], "tamd_op_supported": [ci, ci],
        }.items():
            getattr(L, name).argtypes = args
        L.tamd_graph_destroy.restype = None
        L.tamd_lut_table.argtypes = [ci, ci, vp, C.c_float, ci, C.c_float, ci, C.POINTER(C.c_ubyte)]
        if hasattr(L, "tamd_eltwise_table"):      # (guarded like the slots: an older build has no Eltwise tables)
            L.tamd_eltwise_table.argtypes = [ci, ci, vp, C.c_float, C.c_float, ci, C.c_float, ci, C.POINTER(C.c_ubyte)]
            L.tamd_eltwise_scalar.argtypes = [ci, vp, C.c_float, ci, C.POINTER(C.c_float)]
            L.tamd_eltwise_pair.argtypes = [ci, ci, C.c_ubyte, C.c_float, ci, C.c_ubyte, C.c_float, ci, C.c_float, ci]
            L.tamd_graph_bytemap_chain.argtypes = [vp, ci, C.POINTER(ci), ci, C.POINTER(C.c_ubyte)]
            L.tamd_batchnorm_table.argtypes = [vp] + [C.c_float] * 5 + [ci, C.c_float, ci, C.POINTER(C.c_ubyte)]
        L.tamd_interp_table.argtypes = [ci, C.c_float, ci, C.c_float, ci, C.POINTER(C.c_ubyte)]
        L.tamd_interp_indices.argtypes = [ci, ci, C.c_float, C.POINTER(ci)]
        if hasattr(L, "tamd_resize_table"):       # (guarded like the slots: an older build has no Resize)
            L.tamd_resize_table.argtypes = [ci, C.c_float, ci, C.c_float, ci, C.POINTER(C.c_ubyte)]
            L.tamd_resize_indices.argtypes = [ci, ci, C.c_float, C.POINTER(ci)]
        if hasattr(L, "tamd_instancenorm_plane"):     # (guarded like the slots: an older build has no InstanceNorm)
            L.tamd_instancenorm_plane.argtypes = [C.POINTER(C.c_ubyte), ci] + [C.c_float] * 4 + [ci, C.c_float, ci, C.POINTER(C.c_ubyte), C.POINTER(C.c_float)]
            L.tamd_graph_instancenorm_plan.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci)]
        L.tamd_shuffle_sources.argtypes = [ci, ci, C.POINTER(ci)]
        L.tamd_split_table.argtypes = [C.c_float, ci, C.c_float, ci, C.POINTER(C.c_ubyte)]
        L.tamd_slice_table.argtypes = [C.c_float, ci, C.c_float, ci, C.POINTER(C.c_ubyte)]
        L.tamd_transpose_table.argtypes = [ci, C.c_float, ci, C.c_float, ci, C.POINTER(C.c_ubyte)]
        L.tamd_prelu_slope.argtypes = [C.c_ushort]
        L.tamd_prelu_slope.restype = C.c_float
        L.tamd_prelu_table.argtypes = [ci, C.c_ushort, C.c_float, ci, C.c_float, ci, C.POINTER(C.c_ubyte)]
        _lib = L
    return _lib


OP_SIGMOID, OP_CLIP, OP_HARDSWISH, OP_MISH = 16, 17, 18, 19      # TAMD_OP_* of the byte-map operators
OP_INTERP = 20
OP_SPLIT, OP_SHUFFLECHANNEL = 22, 23
OP_PRELU = 25          # (24: reserved, like 21)
OP_SLICE = 26


class SliceParam(C.Structure):        # tamd_slice_param
    _fields_ = [(k, C.c_int) for k in ("axis", "begin", "end", "step", "iscaffe", "ismxnet", "isonnx", "slice_point_num", "begin_num", "size_num")]


def slice_table(in_scale, in_zp, out_scale, out_zp):
    """tamd_slice_table(): the 256 output bytes of a uint8 Slice between tensors of these quantisation parameters; None where the
    reference's conversion to int is undefined.  Needs no GPU."""
    tab = (C.c_ubyte * 256)()
    rc = lib().tamd_slice_table(in_scale, in_zp, out_scale, out_zp, tab)
    return None if rc != 0 else np.frombuffer(tab, dtype=np.uint8).copy()
OP_TRANSPOSE = 28        # (27: reserved, like 21 and 24)
OP_CROP = 30             # (29: reserved too)
OP_DEPTHTOSPACE = 34     # (33: reserved too)


class DepthToSpaceParam(C.Structure):  # tamd_depthtospace_param
    _fields_ = [("block_size", C.c_int)]
OP_RESIZE = 36           # (35: reserved too)


class ResizeParam(C.Structure):       # tamd_resize_param
    _fields_ = [("scale_w", C.c_float), ("scale_h", C.c_float), ("type", C.c_int)]


def resize_table(dtype, in_scale, in_zp, out_scale, out_zp):
    """tamd_resize_table(): the 256 output bytes (uint8 array, indexed by the input byte's bit pattern) of a nearest Resize node between
    tensors of these quantisation parameters; None for a type the device does not run and where the reference's conversion to int is
    undefined.  Needs no GPU."""
    tab = (C.c_ubyte * 256)()
    rc = lib().tamd_resize_table(dtype, in_scale, in_zp, out_scale, out_zp, tab)
    return None if rc != 0 else np.frombuffer(tab, dtype=np.uint8).copy()


def resize_indices(in_extent, out_extent, scale):
    """tamd_resize_indices(): the source row (column) of every output row (column) of a nearest Resize node whose scale_h (scale_w) is
    `scale`: min((int)(o * (1.f / scale)), in_extent - 1); None for a scale that is not finite and positive.  Needs no GPU."""
    idx = (C.c_int * max(out_extent, 1))()
    rc = lib().tamd_resize_indices(in_extent, out_extent, scale, idx)
    return None if rc != 0 else np.array(idx[:out_extent], dtype=np.int32)


OP_INSTANCENORM = 38     # (37: reserved too)


class InstanceNormParam(C.Structure): # tamd_instancenorm_param
    _fields_ = [("eps", C.c_float)]


def instancenorm_plane(x, gamma, beta, eps, in_scale, in_zp, out_scale, out_zp):
    """tamd_instancenorm_plane(): (rc, the 256-entry byte map of ONE plane of a uint8 InstanceNorm, [sum, sqsum, a, b] as float32) for the
    plane's bytes x (any shape, read in order).  rc -2: a value is NaN or outside int.  The map and the statistics are None unless rc is 0.  Needs no GPU."""
    xb = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
    tab, st = (C.c_ubyte * 256)(), (C.c_float * 4)()
    rc = lib().tamd_instancenorm_plane(xb.ctypes.data_as(C.POINTER(C.c_ubyte)), xb.size, gamma, beta, eps, in_scale, in_zp, out_scale, out_zp, tab, st)
    if rc != 0:
        return rc, None, None
    return 0, np.frombuffer(tab, dtype=np.uint8).copy(), np.array(st[:], dtype=np.float32)


def instancenorm_plan(tm_bytes, node):
    """tamd_graph_instancenorm_plan() of the model's node `node` (its index in the file): (form -- 1 up to 4096 bytes a plane, 0 above, or what
    TAMD_PIN=instnorm_form says --, index of the ReLU node composed into the
    map or -1: an upper bound, asked before buffers are planned), or None where that node is no InstanceNorm the device runs.  Needs no GPU."""
    L = lib()
    h = L.tamd_graph_load_tm2(tm_bytes, len(tm_bytes))
    if not h:
        raise TamdError("load_tm2 failed: %s" % L.tamd_last_error().decode())
    try:
        form, relu = C.c_int(), C.c_int()
        rc = L.tamd_graph_instancenorm_plan(h, node, C.byref(form), C.byref(relu))
        return None if rc != 0 else (form.value, relu.value)
    finally:
        L.tamd_graph_destroy(h)


class CropParam(C.Structure):         # tamd_crop_param
    _fields_ = [(k, C.c_int) for k in ("num_args", "offset_c", "offset_h", "offset_w", "crop_h", "crop_w", "center_crop", "axis", "flag")]


class TransposeParam(C.Structure):    # tamd_transpose_param
    _fields_ = [("dim_num", C.c_int), ("order", C.c_int * 8)]


def transpose_table(dtype, in_scale, in_zp, out_scale, out_zp):
    """tamd_transpose_table(): the 256 output bytes of a Transpose (dtype 2: int8, 3: uint8) between tensors of these quantisation
    parameters, indexed by the raw input byte; the dtype's numpy type (int8: two's complement), so that table[x.view(np.uint8)] are the
    output's values.  None where the reference's conversion to int is undefined.  Needs no GPU."""
    tab = (C.c_ubyte * 256)()
    rc = lib().tamd_transpose_table(dtype, in_scale, in_zp, out_scale, out_zp, tab)
    return None if rc != 0 else np.frombuffer(tab, dtype=np.uint8).copy().view(np.int8 if dtype == 2 else np.uint8)


SPLIT_MAX = 8


class SplitParam(C.Structure):        # tamd_split_param
    _fields_ = [("axis", C.c_int), ("num", C.c_int), ("sizes", C.c_int * SPLIT_MAX)]


class ShuffleChannelParam(C.Structure):   # tamd_shufflechannel_param
    _fields_ = [("group", C.c_int)]


def shuffle_sources(channels, group):
    """tamd_shuffle_sources(): the input channel every output channel of a ShuffleChannel node takes; None when the group count does not
    divide the channels.  Needs no GPU."""
    src = (C.c_int * max(channels, 1))()
    rc = lib().tamd_shuffle_sources(channels, group, src)
    return None if rc != 0 else np.array(src[:channels], dtype=np.int32)


def prelu_slope(half_bits):
    """tamd_prelu_slope(): the float the reference makes of one fp16 slope (bit pattern) -- not IEEE: an exact power of two gives +0.0.
    Needs no GPU."""
    return float(lib().tamd_prelu_slope(int(half_bits) & 0xffff))


def prelu_table(dtype, slope_bits, in_scale, in_zp, out_scale, out_zp):
    """tamd_prelu_table(): the 256 output bytes (uint8 array, indexed by the input byte's bit pattern) of one channel of a PReLU node
    whose fp16 slope has these bits, between tensors of these quantisation parameters; None for a type other than int8 / uint8 and for
    a slope that widens to inf or NaN.  Needs no GPU."""
    tab = (C.c_ubyte * 256)()
    rc = lib().tamd_prelu_table(dtype, int(slope_bits) & 0xffff, in_scale, in_zp, out_scale, out_zp, tab)
    return None if rc != 0 else np.frombuffer(tab, dtype=np.uint8).copy()


def split_table(in_scale, in_zp, out_scale, out_zp):
    """tamd_split_table(): the 256 output bytes of a uint8 Split between tensors of these quantisation parameters.  Needs no GPU."""
    tab = (C.c_ubyte * 256)()
    rc = lib().tamd_split_table(in_scale, in_zp, out_scale, out_zp, tab)
    return None if rc != 0 else np.frombuffer(tab, dtype=np.uint8).copy()


def interp_table(dtype, in_scale, in_zp, out_scale, out_zp):
    """tamd_interp_table(): the 256 output bytes (uint8 array, indexed by the input byte's bit pattern) of a nearest Interp node between
    tensors of these quantisation parameters; None for a type the device does not run.  Needs no GPU."""
    tab = (C.c_ubyte * 256)()
    rc = lib().tamd_interp_table(dtype, in_scale, in_zp, out_scale, out_zp, tab)
    return None if rc != 0 else np.frombuffer(tab, dtype=np.uint8).copy()


def interp_indices(in_extent, out_extent, scale):
    """tamd_interp_indices(): the source row (column) of every output row (column) of a nearest Interp node, (int)((float)o / scale);
    None when one of them leaves the input.  Needs no GPU."""
    idx = (C.c_int * max(out_extent, 1))()
    rc = lib().tamd_interp_indices(in_extent, out_extent, scale, idx)
    return None if rc != 0 else np.array(idx[:out_extent], dtype=np.int32)


def lut_table(op, dtype, in_scale, in_zp, out_scale, out_zp, params=None):
    """tamd_lut_table(): the 256 output bytes (uint8 array, indexed by the input byte's bit pattern) the device applies for a Sigmoid /
    Clip / HardSwish / Mish node between tensors of these quantisation parameters; None for a pair the device does not run.  `params`:
    the node's two floats (Clip: max, min; HardSwish: alpha, beta).  Needs no GPU."""
    tab = (C.c_ubyte * 256)()
    p = (C.c_float * 2)(*params) if params is not None else None
    rc = lib().tamd_lut_table(op, dtype, C.cast(p, C.c_void_p) if p is not None else None, in_scale, in_zp, out_scale, out_zp, tab)
    return None if rc != 0 else np.frombuffer(tab, dtype=np.uint8).copy()


class EltwiseParam(C.Structure):        # tamd_eltwise_param
    _fields_ = [("type", C.c_int), ("caffe_flavor", C.c_int), ("shift", C.c_float), ("power", C.c_float), ("scale", C.c_float)]


def eltwise_scalar(const_dtype, value, scale=0.0, zp=0):
    """tamd_eltwise_scalar(): the float the reference's quantised Eltwise kernels make of a one-element constant (a numpy scalar or array
    of the constant's own type: float32 as it is, uint8 (u - zp) * scale, int8 q * scale); None for another type"""
    v = np.ascontiguousarray(value).reshape(-1)[:1]
    out = C.c_float()
    rc = lib().tamd_eltwise_scalar(const_dtype, v.ctypes.data_as(C.c_void_p), scale, zp, C.byref(out))
    return None if rc != 0 else out.value


def eltwise_table(typ, dtype, scalar, in_scale, in_zp, out_scale, out_zp, shift=0.0, power=1.0, scale=1.0):
    """tamd_eltwise_table(): (rc, the 256 output bytes) of an Eltwise node with a constant one-element second operand (`scalar`, already a
    float: eltwise_scalar) or of a unary type (shift / power / scale: POWER 17 reads them).  rc 0; -1: no such (type, dtype) on the
    device; -2: the table holds a value the reference does not define.  The bytes are None unless rc is 0.  Needs no GPU."""
    tab = (C.c_ubyte * 256)()
    p = EltwiseParam(typ, 0, shift, power, scale)
    rc = lib().tamd_eltwise_table(typ, dtype, C.cast(C.pointer(p), C.c_void_p), scalar, in_scale, in_zp, out_scale, out_zp, tab)
    return rc, (np.frombuffer(tab, dtype=np.uint8).copy() if rc == 0 else None)


class BatchNormParam(C.Structure):      # tamd_batchnorm_param
    _fields_ = [("rescale_factor", C.c_float), ("eps", C.c_float), ("caffe_flavor", C.c_int)]


def batchnorm_table(gamma, beta, mean, var, in_scale, in_zp, out_scale, out_zp, rescale_factor=1.0, eps=1e-5, caffe_flavor=0):
    """tamd_batchnorm_table(): (rc, the 256 output bytes of ONE channel of a uint8 BatchNorm); rc -2: s1 / s2 or the table is not
    finite.  The bytes are None unless rc is 0.  Needs no GPU."""
    tab = (C.c_ubyte * 256)()
    p = BatchNormParam(rescale_factor, eps, caffe_flavor)
    rc = lib().tamd_batchnorm_table(C.cast(C.pointer(p), C.c_void_p), gamma, beta, mean, var, in_scale, in_zp, out_scale, out_zp, tab)
    return rc, (np.frombuffer(tab, dtype=np.uint8).copy() if rc == 0 else None)


def eltwise_pair(typ, dtype, a, qa, b, qb, qo):
    """tamd_eltwise_pair(): the output byte of the same-shape PROD / SUM / SUB / MAX on one pair of bytes (q*: (scale, zero point)); < 0
    as the C function answers"""
    return lib().tamd_eltwise_pair(typ, dtype, int(a) & 255, qa[0], int(qa[1]), int(b) & 255, qb[0], int(qb[1]), qo[0], int(qo[1]))


def bytemap_chain(tm_bytes, node):
    """tamd_graph_bytemap_chain() of the model's node `node` (its index in the file): (member node indices, the 256-byte table from the
    chain's source tensor to its last tensor), or ([], None) where no chain starts.  Needs no GPU."""
    L = lib()
    h = L.tamd_graph_load_tm2(tm_bytes, len(tm_bytes))
    if not h:
        raise TamdError("load_tm2 failed: %s" % L.tamd_last_error().decode())
    try:
        nodes, tab = (C.c_int * 64)(), (C.c_ubyte * 256)()
        n = L.tamd_graph_bytemap_chain(h, node, nodes, 64, tab)
        if n < 0:
            raise TamdError("bytemap_chain: bad arguments")
        return (list(nodes[:n]), np.frombuffer(tab, dtype=np.uint8).copy()) if n else ([], None)
    finally:
        L.tamd_graph_destroy(h)


def _check(rc, what):
    if rc is None or (isinstance(rc, int) and rc < 0):
        raise TamdError("%s failed: %s" % (what, lib().tamd_last_error().decode()))
    return rc


def device_count():
    return lib().tamd_device_count()


class Graph:
    """A device graph loaded from tmfile bytes (same bytes the reference's `tengine:m` loader takes)."""

    def __init__(self, tm_bytes: bytes, batch=None, gpu_index=0, use_hip_graph=True, profile=False, direct_dispatch=False, keep_tensors=False, u8_integer=False, split_batch=0):
        L = lib()
        self._h = L.tamd_graph_load_tm2(tm_bytes, len(tm_bytes))
        if not self._h:
            raise TamdError("tamd_graph_load_tm2 failed: %s" % L.tamd_last_error().decode())
        if batch is not None:
            _check(L.tamd_graph_set_batch(self._h, batch), "set_batch")
        opt = Options(b"HIP", C.sizeof(Options), gpu_index, 1 if use_hip_graph else 0, 1 if profile else 0, 1 if direct_dispatch else 0,
                      1 if keep_tensors else 0, 1 if u8_integer else 0, int(split_batch))
        _check(L.tamd_graph_prerun(self._h, C.byref(opt)), "prerun")
        self._in, self._out = [], []
        for i in range(L.tamd_graph_output_num(self._h)):
            dims = (C.c_int * 8)()
            dt, sc, zp = C.c_int(), C.c_float(), C.c_int()
            nd = L.tamd_graph_output_desc(self._h, i, dims, C.byref(dt), C.byref(sc), C.byref(zp))
            arr = np.zeros([dims[k] for k in range(nd)], _NP[dt.value])
            self._out.append(arr)
            _check(L.tamd_graph_set_output(self._h, i, arr.ctypes.data, arr.nbytes), "set_output")

    def halves(self):
        """2: compiled as two half-batch device graphs behind this one handle (tamd_options.split_batch); 0: one launch list"""
        return lib().tamd_graph_halves(self._h)

    def slots(self):
        """2: launch() keeps two passes of the launch list in flight on two HSA queues (tamd_options.split_batch, two slots); 0: one at a time"""
        return lib().tamd_graph_slots(self._h) if hasattr(lib(), "tamd_graph_slots") else 0

    def slot_timestamps(self, passes=50):
        """one burst of `passes` rounds of (a pass on slot 0's queue, a pass on slot 1's), every packet stamped: (start_us, end_us), two
        float arrays of shape [rounds, 2, packets] on the common clock, counted from the earliest start"""
        n = lib().tamd_graph_direct_packets(self._h)
        t0, t1 = (C.c_double * (passes * 2 * n))(), (C.c_double * (passes * 2 * n))()
        r = _check(lib().tamd_graph_slot_timestamps(self._h, passes, t0, t1, passes * 2 * n), "slot_timestamps")
        return (np.array(t0[:r * 2 * n]).reshape(r, 2, n), np.array(t1[:r * 2 * n]).reshape(r, 2, n))

    def input_desc(self, idx=0):
        dims = (C.c_int * 8)()
        dt = C.c_int()
        nd = lib().tamd_graph_input_desc(self._h, idx, dims, C.byref(dt))
        return [dims[k] for k in range(nd)], dt.value

    def set_input(self, arr, idx=0):
        arr = np.ascontiguousarray(arr)
        while len(self._in) <= idx:
            self._in.append(None)
        self._in[idx] = arr       # keep alive: the pointer is re-read at every run
        _check(lib().tamd_graph_set_input(self._h, idx, arr.ctypes.data, arr.nbytes), "set_input")

    def run(self):
        _check(lib().tamd_graph_run(self._h), "run")
        return [o.copy() for o in self._out]

    def run_noreturn(self):
        """tamd_graph_run() without copying the outputs again (they are in the arrays handed to set_output)"""
        _check(lib().tamd_graph_run(self._h), "run")

    def run_async(self, out_arrays=None):
        """tamd_graph_run_async(): submit the current input; `out_arrays` (one per output) receive THIS run's results at wait()"""
        if out_arrays is not None:
            for i, a in enumerate(out_arrays):
                _check(lib().tamd_graph_set_output(self._h, i, a.ctypes.data, a.nbytes), "set_output")
        _check(lib().tamd_graph_run_async(self._h), "run_async")

    def wait(self):
        _check(lib().tamd_graph_wait(self._h), "wait")

    def bind_default_outputs(self):
        """point the graph's output buffers back at the arrays run() / download() return"""
        for i, a in enumerate(self._out):
            _check(lib().tamd_graph_set_output(self._h, i, a.ctypes.data, a.nbytes), "set_output")

    def output_like(self):
        return [np.zeros_like(o) for o in self._out]

    def output_num(self):
        return lib().tamd_graph_output_num(self._h)

    def upload(self):
        _check(lib().tamd_graph_upload_inputs(self._h), "upload_inputs")

    def launch(self):
        _check(lib().tamd_graph_launch(self._h), "launch")

    def sync(self):
        _check(lib().tamd_graph_sync(self._h), "sync")

    def download(self):
        _check(lib().tamd_graph_download_outputs(self._h), "download_outputs")
        return [o.copy() for o in self._out]

    def time_launches(self, iters):
        ms = C.c_float()
        _check(lib().tamd_graph_time_launches(self._h, iters, C.byref(ms)), "time_launches")
        return ms.value

    def output_device(self, idx=0):
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().tamd_graph_output_device(self._h, idx, C.byref(p), C.byref(n)), "output_device")
        return p.value, n.value

    def stream(self):
        return lib().tamd_graph_stream(self._h)

    def prerun_ms(self):
        """wall milliseconds tamd_graph_prerun took (planning incl. autotune, capture, direct-dispatch programs)"""
        return lib().tamd_graph_prerun_ms(self._h)

    def direct_packets(self):
        """AQL packets per launch() when direct dispatch is active, else 0"""
        return lib().tamd_graph_direct_packets(self._h)

    def direct_timestamps(self, passes=200):
        """the directly dispatched pass under the HSA runtime's dispatch profiling: [(kernel symbol, mean us, mean gap to the next packet us)]"""
        n = lib().tamd_graph_direct_packets(self._h)
        dur, gap = (C.c_double * n)(), (C.c_double * n)()
        _check(lib().tamd_graph_direct_timestamps(self._h, passes, dur, gap, n), "direct_timestamps")
        return [(lib().tamd_graph_direct_packet_name(self._h, i).decode(), dur[i], gap[i]) for i in range(n)]

    def direct_meta_packets(self):
        return lib().tamd_graph_direct_meta_packets(self._h)

    def kernel_num(self):
        """number of compute launches of one forward pass"""
        return lib().tamd_graph_kernel_num(self._h)

    def profile(self, iters=10):
        n = lib().tamd_graph_kernel_num(self._h)
        arr = (KernelInfo * n)()
        _check(lib().tamd_graph_profile(self._h, iters, arr, n), "profile")
        return [dict(node=k.node.decode(), kernel=k.kernel.decode(), macs=k.macs, bytes=k.bytes, ms=k.ms) for k in arr]

    def read_tensor(self, idx):
        dims = (C.c_int * 8)()
        dt = C.c_int()
        nd = _check(lib().tamd_graph_tensor_desc(self._h, idx, dims, C.byref(dt)), "tensor_desc")
        arr = np.zeros([dims[k] for k in range(nd)], _NP[dt.value])
        _check(lib().tamd_graph_read_tensor(self._h, idx, arr.ctypes.data, arr.nbytes), "read_tensor")
        return arr

    def close(self):
        if self._h:
            lib().tamd_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
