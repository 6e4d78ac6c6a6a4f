"""mi355fx — ctypes binding of libmi355fx.so (the C ABI of include/mi355fx.h).

This is plumbing for tests/, bench.py and __graft_entry__.py: it loads the in-tree shared library
built by gst-plugins-rs_amd/Makefile and exposes its entry points 1:1. There is NO fallback: if the
library is missing the import raises, and on a box without a gfx950 device Context() raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("MI355FX_LIB") or os.path.join(PKG_ROOT, "libmi355fx.so")   # MI355FX_LIB: an experimental build (tools/)
HEADER_PATH = os.path.join(os.path.dirname(PKG_ROOT), "include", "mi355fx.h")

# mi355_video_format
FMT = {"RGBx": 0, "xRGB": 1, "BGRx": 2, "xBGR": 3, "RGBA": 4, "ARGB": 5, "BGRA": 6, "ABGR": 7,
       "RGB": 8, "BGR": 9, "RGBA64_LE": 10, "RGBA64_BE": 11}
# (pixel_stride, first, bgr) per format — mirrors the match arms of video/hsv/src/hsvfilter/imp.rs:327-373
FMT_LAYOUT = {"RGBx": (4, 0, 0), "RGBA": (4, 0, 0), "RGB": (3, 0, 0), "xRGB": (4, 1, 0), "ARGB": (4, 1, 0),
              "BGRx": (4, 0, 1), "BGRA": (4, 0, 1), "BGR": (3, 0, 1), "xBGR": (4, 1, 1), "ABGR": (4, 1, 1)}

OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_NOT_CONFIGURED, ERR_OOM, ERR_UNSUPPORTED, ERR_TIMEOUT = 0, -1, -2, -3, -4, -5, -6, -7
FLAG_FORCE_GENERIC = 1
FLAG_HSV_BLOCKS_PER_CU = 2
FLAG_FUSED_VARIANT = 3
FLAG_LUT_VARIANT = 4
FLAG_LUT_STAGGER = 5
FLAG_HSV_TABLE = 6
FLAG_BRICK_TILES_PER_RUN = 7
FLAG_BRICK_SETS = 8
FLAG_BRICK_PRIO = 9
FLAG_BRICK_FOLD_AXIS = 10
FLAG_DSSIM_TRANSLUCENT = 11
FLAG_HRTF_METHOD = 12
FLAG_WINDOW_MIN_STEPS = 13
FLAG_HSV_NT = 14
FLAG_BLOCKHASH_ANY_SIZE = 15
FLAG_WINDOW_ORDER = 17
FLAG_WINDOW_STATS = 18
FLAG_DSSIM_FAST = 19
HSVDETECT_SET_MAX = 32   # MI355_HSVDETECT_SET_MAX: detector frames per launch set of a Group
HSVFILTER_SET_MAX = 32   # MI355_HSVFILTER_SET_MAX: hsvfilter frames per launch set of a Group
COLORLUT_SET_MAX = 32    # MI355_COLORLUT_SET_MAX: colorlut frames per launch set of a Group
YOLODEC_SET_MAX = 32     # MI355_YOLODEC_SET_MAX: decoder tensors per launch set of a Group
MIXER_FRAME_TILE = 64    # MI355_MIXER_FRAME_TILE: frames per block of the mixer kernel


class HsvSettings(C.Structure):
    _fields_ = [("hue_shift", C.c_float), ("saturation_mul", C.c_float), ("saturation_off", C.c_float),
                ("value_mul", C.c_float), ("value_off", C.c_float)]


class HsvFilterPlanFrame(C.Structure):
    """mi355_hsvfilter_plan_frame: one frame as mi355_selftest_hsvfilter_set_plan takes it; the address is a number."""
    _fields_ = [("address", C.c_uint64), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("format", C.c_int32),
                ("settings", HsvSettings), ("force_generic", C.c_int32)]


class HsvFilterPlanOut(C.Structure):
    """mi355_hsvfilter_plan_out: where the builder puts a frame (launch: 0 no pixel, 1 vector, 2 literal)."""
    _fields_ = [("set", C.c_int32), ("launch", C.c_int32), ("variant", C.c_int32), ("first_block", C.c_uint32), ("blocks", C.c_uint32),
                ("reserved", C.c_uint32), ("units", C.c_uint64)]


class ColorLutPlanFrame(C.Structure):
    """mi355_colorlut_plan_frame: one frame as mi355_selftest_colorlut_set_plan takes it; the addresses are numbers."""
    _fields_ = [("src_address", C.c_uint64), ("dst_address", C.c_uint64), ("src_stride", C.c_int32), ("dst_stride", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("format", C.c_int32), ("force_generic", C.c_int32)]


class ColorLutPlanOut(C.Structure):
    """mi355_colorlut_plan_out: where the builder puts a frame (launch: 0 no pixel, 1 vector, 2 literal; geometry: 1 flat, 2 rowpad)."""
    _fields_ = [("set", C.c_int32), ("launch", C.c_int32), ("geometry", C.c_int32), ("first_block", C.c_uint32), ("blocks", C.c_uint32),
                ("reserved", C.c_uint32), ("units", C.c_uint64)]


class DssimPlan(C.Structure):
    """mi355_dssim_plan: the exact Dssim engine's geometry of one frame size (mi355_selftest_dssim_plan)."""
    _fields_ = [("tile_w", C.c_int32), ("tile_h", C.c_int32), ("tile_lanes", C.c_int32), ("scale_halo", C.c_int32), ("compare_halo", C.c_int32),
                ("n_scales", C.c_int32), ("w", C.c_int32 * 5), ("h", C.c_int32 * 5),
                ("tiles", C.c_uint32 * 5), ("interior_scale", C.c_uint32 * 5), ("interior_compare", C.c_uint32 * 5),
                ("n_launches", C.c_int32), ("launch_scale", C.c_int32 * 3), ("launch_jobs", C.c_int32 * 3), ("launch_first", (C.c_uint32 * 4) * 3),
                ("downsample_blocks", C.c_uint32 * 5), ("absdev_blocks", C.c_uint32 * 5), ("avg_blocks", C.c_uint32), ("sum_blocks", C.c_uint32)]


class AgingRadioSettings(C.Structure):
    """mi355_agingradio_settings: agingradio's Settings as transform_ip snapshots them (lowpass-freq goes to setup)."""
    _fields_ = [("white_noise_ampl", C.c_float), ("clicks_prob", C.c_float), ("bits_to_quantize", C.c_float),
                ("cubic_curve_distortion", C.c_float), ("cubic_curve_passes", C.c_uint32)]

    @classmethod
    def of(cls, d):
        return cls(d.get("white_noise_ampl", 0.011), d.get("clicks_prob", 1.0 / 100000.0), d.get("bits_to_quantize", 4.0),
                   d.get("cubic_curve_distortion", 1.0), d.get("cubic_curve_passes", 3))


class MixerSegment(C.Structure):
    """mi355_mixer_segment: num_frames mono frames of input pad `input` (format 0 F32LE, 1 S16LE) landing at output frame out_offset."""
    _fields_ = [("data", C.c_void_p), ("input", C.c_uint32), ("format", C.c_uint32), ("out_offset", C.c_uint32), ("num_frames", C.c_uint32)]


class MixerOutput(C.Structure):
    """mi355_mixer_output: an interleaved buffer of frames x n_channels samples fed by the channels from channel_offset on."""
    _fields_ = [("data", C.c_void_p), ("format", C.c_uint32), ("channel_offset", C.c_uint32), ("n_channels", C.c_uint32)]


def mixer_tables(segments, outputs):
    """The arrays of a mixer call. segments: (input, data, out_offset) with data a 1-D numpy float32 / int16 array, or
    (input, (pointer, format, num_frames), out_offset) for device memory; outputs: (data, channel_offset, n_channels) with data a
    numpy float32 / int16 array of frames * n_channels samples, or ((pointer, format), channel_offset, n_channels).
    -> (MixerSegment array, MixerOutput array); the caller keeps the numpy arrays alive."""
    fmt = {np.dtype(np.float32): 0, np.dtype(np.int16): 1}
    segs = (MixerSegment * max(len(segments), 1))()
    for k, (inp, data, off) in enumerate(segments):
        if isinstance(data, np.ndarray):
            assert data.ndim == 1 and data.flags.c_contiguous
            segs[k] = MixerSegment(data.ctypes.data if data.size else None, inp, fmt[data.dtype], off, data.size)
        else:
            segs[k] = MixerSegment(data[0], inp, data[1], off, data[2])
    outs = (MixerOutput * max(len(outputs), 1))()
    for k, (data, off, nch) in enumerate(outputs):
        if isinstance(data, np.ndarray):
            assert data.flags.c_contiguous
            outs[k] = MixerOutput(data.ctypes.data if data.size else None, fmt[data.dtype], off, nch)
        else:
            outs[k] = MixerOutput(data[0], data[1], off, nch)
    return segs, outs


class YoloParams(C.Structure):
    """mi355_yolo_params: the three thresholds of one yolov8tensordec2 / yoloxtensordec instance."""
    _fields_ = [("box_confidence_threshold", C.c_float), ("class_confidence_threshold", C.c_float), ("iou_threshold", C.c_float)]


YOLO_LAYOUT = {"V8": 0, "X": 1}   # mi355_yolo_layout
YOLO_X_INFER = 3  # MI355_YOLO_X_INFER: an infer member's kind in selftest_yolox_infer_set_plan (no layout of the entry points)
YOLO_X_HEAD = 2   # MI355_YOLO_X_HEAD: a head member's kind in selftest_yolox_head_set_plan (no layout of the entry points)
# mi355_yolo_det as a numpy record
YOLO_DET = np.dtype([("xmin", "<f4"), ("ymin", "<f4"), ("xmax", "<f4"), ("ymax", "<f4"), ("x", "<i4"), ("y", "<i4"), ("width", "<i4"),
                     ("height", "<i4"), ("class_id", "<u4"), ("confidence", "<f4"), ("candidate", "<u4"), ("reserved", "<u4")])


def _yolo_params(params):
    """One (box_thr, class_thr, iou_thr) triple, a YoloParams, or a sequence of either -> a ctypes array."""
    if isinstance(params, YoloParams) or (len(params) == 3 and not hasattr(params[0], "__len__") and not isinstance(params[0], YoloParams)):
        params = [params]
    arr = (YoloParams * max(len(params), 1))()
    for k, q in enumerate(params):
        arr[k] = q if isinstance(q, YoloParams) else YoloParams(*[float(v) for v in q])
    return arr, len(params)


YOLOX_LEVELS_MAX = 8   # MI355_YOLOX_LEVELS_MAX


class YoloxLevel(C.Structure):
    """mi355_yolox_level: one level of a YOLOX head - tensor 0's reg [4][h][w], obj [1][h][w] and cls [C][h][w] maps (tensor i's at
    pointer + i * pitch), the level's shape and its stride."""
    _fields_ = [("reg", C.c_void_p), ("obj", C.c_void_p), ("cls", C.c_void_p), ("reg_pitch_bytes", C.c_size_t), ("obj_pitch_bytes", C.c_size_t),
                ("cls_pitch_bytes", C.c_size_t), ("h", C.c_uint32), ("w", C.c_uint32), ("stride", C.c_uint32), ("reserved", C.c_uint32)]


def _yolox_levels(levels):
    """YoloxLevel objects, or tuples (reg, obj, cls, reg_pitch, obj_pitch, cls_pitch, h, w, stride[, reserved]) -> a ctypes array."""
    arr = (YoloxLevel * max(len(levels), 1))()
    for k, q in enumerate(levels):
        arr[k] = q if isinstance(q, YoloxLevel) else YoloxLevel(*q)
    return arr


def yolox_candidates(levels):
    """A = the sum of h * w over the levels (YoloxLevel objects or the tuples _yolox_levels takes)."""
    return sum((q.h * q.w) if isinstance(q, YoloxLevel) else (q[6] * q[7]) for q in levels)



class YoloxNetConfig(C.Structure):
    """mi355_yolox_net_config: depth, width, depthwise, num_classes of a YOLOX network; reserved 0."""
    _fields_ = [("depth", C.c_double), ("width", C.c_double), ("depthwise", C.c_int32), ("num_classes", C.c_uint32), ("reserved", C.c_uint32)]


# the reference's six constructors (MI355_YOLOX_NET_NANO .. _X): (depth, width, depthwise)
YOLOX_VARIANTS = {"nano": (0.33, 0.25, True), "tiny": (0.33, 0.375, False), "s": (0.33, 0.50, False), "m": (0.67, 0.75, False), "l": (1.0, 1.0, False),
                  "x": (1.33, 1.25, False)}
YOLOX_NET_MAX_FRAMES, YOLOX_NET_MAX_SIDE, YOLOX_NET_NAME_MAX = 64, 2048, 96
YOLOX_PRECISION = {"f32": 0, "bf16": 1}   # MI355_YOLOX_PRECISION_*
YOLOX_OP = {"conv": 0, "dw": 1, "pool5": 2, "up2": 3, "focus": 4}   # kinds of mi355_selftest_yolox_net_op_device


def yolox_net_config(depth, width, depthwise, num_classes, reserved=0):
    return YoloxNetConfig(float(depth), float(width), int(depthwise), int(num_classes), int(reserved))


class YoloxNetPlan(C.Structure):
    """mi355_yolox_net_plan: what mi355_selftest_yolox_net_plan reports."""
    _fields_ = [("status", C.c_int32), ("config_status", C.c_int32), ("frames_status", C.c_int32), ("size_status", C.c_int32), ("param_count", C.c_uint32),
                ("launches", C.c_uint32), ("param_floats", C.c_uint64), ("arena_bytes", C.c_uint64), ("macs", C.c_uint64), ("level_h", C.c_uint32 * 3),
                ("level_w", C.c_uint32 * 3)]


class YoloxNetOp(C.Structure):
    """mi355_yolox_net_op: one op on caller views (mi355_selftest_yolox_net_op_device)."""
    _fields_ = [("kind", C.c_int32), ("k", C.c_int32), ("stride", C.c_int32), ("silu", C.c_int32), ("n_frames", C.c_uint32), ("h_in", C.c_uint32),
                ("w_in", C.c_uint32), ("tile", C.c_uint32), ("inp", C.c_void_p), ("in_c", C.c_uint32), ("in_off", C.c_uint32), ("in_ctot", C.c_uint32),
                ("out_c", C.c_uint32), ("out", C.c_void_p), ("out_off", C.c_uint32), ("out_ctot", C.c_uint32), ("res_off", C.c_uint32),
                ("res_ctot", C.c_uint32), ("res", C.c_void_p), ("weight", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p)]


class HandParams(C.Structure):
    """mi355_hand_params: the settings of one handdetectiontensordec / handlandmarktensordec instance; frame 0, 0: no frame size."""
    _fields_ = [("confidence_threshold", C.c_float), ("nms_iou_threshold", C.c_float), ("max_hands", C.c_uint32), ("frame_width", C.c_int32),
                ("frame_height", C.c_int32)]


HAND_MAX = 10   # MI355_HAND_MAX: records per tensor in the outputs
HANDDEC_SET_MAX = 32   # MI355_HANDDEC_SET_MAX: tensors per launch set of the group's hand-decoder queue
KP_VISIBILITY = {"UNKNOWN": 0, "VISIBLE": 1, "OCCLUDED": 2}   # mi355_kp_visibility
# mi355_hand_det and mi355_hand_keypoints as numpy records
HAND_DET = np.dtype([("xmin", "<f4"), ("ymin", "<f4"), ("xmax", "<f4"), ("ymax", "<f4"), ("rotation", "<f4"), ("rotation_od", "<f4"), ("confidence", "<f4"),
                     ("index", "<u4"), ("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4"), ("has_od", "<u4"), ("reserved", "<u4", (3,))])
HAND_KP = np.dtype([("count", "<u4"), ("positions", "<i4", (42,)), ("confidences", "<f4", (21,)), ("visibilities", "u1", (21,)), ("reserved", "u1", (11,))])


def _hand_params(params):
    """One (confidence_thr, nms_iou_thr, max_hands[, frame_width, frame_height]) tuple, a HandParams, or a sequence of either -> a
    ctypes array. A missing or None frame size is 0, 0."""
    if isinstance(params, HandParams) or not (hasattr(params[0], "__len__") or isinstance(params[0], HandParams)):
        params = [params]
    arr = (HandParams * max(len(params), 1))()
    for k, q in enumerate(params):
        if isinstance(q, HandParams):
            arr[k] = q
        else:
            frame = tuple(q[3:5]) if len(q) >= 5 and q[3] is not None else (0, 0)
            arr[k] = HandParams(float(q[0]), float(q[1]), int(q[2]), int(frame[0]), int(frame[1]))
    return arr, len(params)


class HsvDetectSettings(C.Structure):
    _fields_ = [("hue_ref", C.c_float), ("hue_var", C.c_float), ("saturation_ref", C.c_float),
                ("saturation_var", C.c_float), ("value_ref", C.c_float), ("value_var", C.c_float)]


class Mi355Error(RuntimeError):
    def __init__(self, status, message):
        super().__init__("mi355fx status %d: %s" % (status, message))
        self.status = status


_lib = None


def load_library():
    """Load libmi355fx.so (built in-tree). Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libmi355fx.so not built: run `make -C %s` (or __graft_entry__.build())" % PKG_ROOT)
    L = C.CDLL(LIB_PATH)
    vp, sz, i, u8p = C.c_void_p, C.c_size_t, C.c_int, C.c_void_p
    f32p = C.POINTER(C.c_float)
    sig = {
        "mi355_abi_version": (i, []),
        "mi355_device_count": (i, []),
        "mi355_ctx_create": (vp, [i, C.POINTER(i)]),
        "mi355_ctx_destroy": (None, [vp]),
        "mi355_ctx_last_error": (C.c_char_p, [vp]),
        "mi355_status_string": (C.c_char_p, [i]),
        "mi355_ctx_stream": (vp, [vp]),
        "mi355_ctx_set_stream": (i, [vp, vp]),
        "mi355_ctx_synchronize": (i, [vp]),
        "mi355_ctx_set_flag": (i, [vp, i, i]),
        "mi355_device_alloc": (vp, [vp, sz]),
        "mi355_device_free": (i, [vp, vp]),
        "mi355_memcpy_h2d": (i, [vp, vp, vp, sz]),
        "mi355_memcpy_d2h": (i, [vp, vp, vp, sz]),
        "mi355_hsv_colorlut_chain_batches_device": (i, [vp, vp, vp, i, i, sz, i, i, i, i, C.POINTER(HsvSettings), i]),
        "mi355_buf_alloc": (vp, [vp, sz]),
        "mi355_buf_ref": (vp, [vp]),
        "mi355_buf_unref": (None, [vp]),
        "mi355_buf_size": (sz, [vp]),
        "mi355_buf_device_ptr": (vp, [vp, vp, i]),
        "mi355_buf_commit": (i, [vp, vp]),
        "mi355_buf_map_host": (vp, [vp, i]),
        "mi355_buf_unmap_host": (i, [vp]),
        "mi355_buf_state": (i, [vp]),
        "mi355_ctx_transfer_counts": (i, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "mi355_roundedcorners_set_mask": (i, [vp, u8p, i, i, i]),
        "mi355_roundedcorners_mask_device": (i, [vp, C.POINTER(vp), C.POINTER(sz), C.POINTER(i)]),
        "mi355_roundedcorners_append_device": (i, [vp, u8p, sz, sz, i]),
        "mi355_colordetect_frame": (i, [vp, u8p, sz, i, i, i, u8p, C.POINTER(C.c_int)]),
        "mi355_colordetect_frames_device": (i, [vp, vp, sz, sz, i, i, i, i, u8p, C.POINTER(C.c_int)]),
        "mi355_colordetect_histogram_device": (i, [vp, vp, sz, i, i, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
        "mi355_selftest_colordetect_mmcq": (i, [vp, vp, i, vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mi355_hsvfilter_frame_ip": (i, [vp, u8p, sz, i, i, i, C.POINTER(HsvSettings)]),
        "mi355_hsvfilter_frames_device": (i, [vp, u8p, i, sz, i, i, i, i, C.POINTER(HsvSettings)]),
        "mi355_hsvdetect_frame": (i, [vp, u8p, sz, i, i, u8p, sz, i, i, i, C.POINTER(HsvDetectSettings)]),
        "mi355_hsvdetect_frames_device": (i, [vp, u8p, sz, i, i, u8p, sz, i, i, i, i, i, C.POINTER(HsvDetectSettings)]),
        "mi355_colorlut_load": (i, [vp, i, sz, f32p, f32p, f32p]),
        "mi355_colorlut_unload": (i, [vp]),
        "mi355_selftest_autopick": (i, [i, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double), i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mi355_selftest_autopick_settled": (i, [i, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int), i, C.POINTER(C.c_int),
                                                C.POINTER(C.c_int)]),
        "mi355_colorlut_kernel_choice": (i, [vp, i, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "mi355_shared_table_count": (i, []),
        "mi355_colorlut_last_kernel": (C.c_char_p, [vp]),
        "mi355_colorlut_brick_stats": (i, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_int), i]),
        "mi355_colorlut_window_stats": (i, [vp, C.POINTER(C.c_uint64), i]),
        "mi355_selftest_brickwatch": (i, [i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), i, C.POINTER(C.c_int)]),
        "mi355_colorlut_frame": (i, [vp, u8p, i, u8p, i, i, i, i]),
        "mi355_colorlut_frames_device": (i, [vp, u8p, sz, i, u8p, sz, i, i, i, i, i]),
        "mi355_hsv_colorlut_frames_device": (i, [vp, u8p, sz, i, u8p, sz, i, i, i, i, C.POINTER(HsvSettings)]),
        "mi355_echo_setup": (i, [vp, sz]),
        "mi355_echo_reset": (i, [vp]),
        "mi355_echo_process_f32": (i, [vp, vp, sz, sz, C.c_double, C.c_double]),
        "mi355_echo_process_f64": (i, [vp, vp, sz, sz, C.c_double, C.c_double]),
        "mi355_echo_process_device": (i, [vp, vp, sz, i, sz, C.c_double, C.c_double]),
        "mi355_echo_get_state": (i, [vp, vp, sz, C.POINTER(sz)]),
        "mi355_echo_setup_batch": (i, [vp, i, sz]),
        "mi355_echo_process_batch_device": (i, [vp, vp, sz, sz, i, vp, vp, vp]),
        "mi355_echo_get_state_batch": (i, [vp, i, vp, sz, C.POINTER(sz)]),
        "mi355_ebur128_setup": (i, [vp, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_int)]),
        "mi355_ebur128_setup_batch": (i, [vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_int)]),
        "mi355_ebur128_add_frames_batch": (i, [vp, vp, sz, i]),
        "mi355_ebur128_add_frames_batch_device": (i, [vp, vp, sz, i]),
        "mi355_ebur128_loudness_batch": (i, [vp, i, C.POINTER(C.c_double)]),
        "mi355_ebur128_peak_batch": (i, [vp, i, C.POINTER(C.c_double)]),
        "mi355_ebur128_reset": (i, [vp]),
        "mi355_ebur128_teardown": (i, [vp]),
        "mi355_ebur128_add_frames": (i, [vp, vp, sz, i]),
        "mi355_ebur128_add_frames_planar": (i, [vp, C.POINTER(vp), sz, i]),
        "mi355_ebur128_loudness_momentary": (i, [vp, C.POINTER(C.c_double)]),
        "mi355_ebur128_loudness_shortterm": (i, [vp, C.POINTER(C.c_double)]),
        "mi355_ebur128_loudness_global": (i, [vp, C.POINTER(C.c_double)]),
        "mi355_ebur128_relative_threshold": (i, [vp, C.POINTER(C.c_double)]),
        "mi355_ebur128_loudness_range": (i, [vp, C.POINTER(C.c_double)]),
        "mi355_ebur128_sample_peak": (i, [vp, C.c_uint, C.POINTER(C.c_double)]),
        "mi355_ebur128_true_peak": (i, [vp, C.c_uint, C.POINTER(C.c_double)]),
        "mi355_loudnorm_setup": (i, [vp, C.c_uint, C.c_double, C.c_double, C.c_double, C.c_double]),
        "mi355_loudnorm_push": (i, [vp, vp, sz, vp, sz, C.POINTER(sz)]),
        "mi355_loudnorm_drain": (i, [vp, vp, sz, C.POINTER(sz), C.POINTER(i)]),
        "mi355_loudnorm_teardown": (i, [vp]),
        "mi355_loudnorm_setup_batch": (i, [vp, C.c_uint, C.c_uint, C.c_double, C.c_double, C.c_double, C.c_double]),
        "mi355_loudnorm_batch_frame_size": (sz, [vp]),
        "mi355_loudnorm_process_batch": (i, [vp, vp, sz, sz, vp, sz, sz, C.POINTER(sz), i, i]),
        "mi355_host_alloc": (vp, [vp, sz]),
        "mi355_host_free": (i, [vp, vp]),
        "mi355_pipe_create": (vp, [vp, i, sz]),
        "mi355_pipe_destroy": (None, [vp]),
        "mi355_pipe_submit_hsvfilter": (i, [vp, u8p, sz, i, i, i, C.POINTER(HsvSettings), C.POINTER(C.c_uint64)]),
        "mi355_pipe_submit_colorlut": (i, [vp, u8p, i, u8p, i, i, i, i, C.POINTER(C.c_uint64)]),
        "mi355_pipe_submit_hsv_colorlut": (i, [vp, u8p, i, u8p, i, i, i, C.POINTER(HsvSettings), C.POINTER(C.c_uint64)]),
        "mi355_pipe_wait": (i, [vp, C.c_uint64]),
        "mi355_pipe_wait_all": (i, [vp]),
        "mi355_videocompare_hash_frame": (i, [vp, u8p, i, i, i, i, i, C.POINTER(C.c_uint64)]),
        "mi355_videocompare_hash_frames_device": (i, [vp, u8p, sz, i, i, i, i, i, i, C.POINTER(C.c_uint64)]),
        "mi355_videocompare_distance": (C.c_double, [i, C.c_uint64, C.c_uint64]),
        "mi355_dssim_create_image": (i, [vp, u8p, i, i, i, i, C.POINTER(vp)]),
        "mi355_dssim_create_image_device": (i, [vp, u8p, i, i, i, i, C.POINTER(vp)]),
        "mi355_dssim_free_image": (None, [vp, vp]),
        "mi355_dssim_compare": (i, [vp, vp, vp, C.POINTER(C.c_double)]),
        "mi355_dssim_compare_frames": (i, [vp, vp, C.POINTER(vp), i, i, i, i, i, C.POINTER(C.c_double)]),
        "mi355_dssim_compare_frames_device": (i, [vp, vp, C.POINTER(vp), i, i, i, i, i, C.POINTER(C.c_double)]),
        "mi355_issue_streams_round": (i, [C.POINTER(vp), i, C.POINTER(vp), C.POINTER(vp), i, i, i, i, C.POINTER(HsvSettings)]),
        "mi355_group_create": (vp, [i, i, C.POINTER(C.c_int)]),
        "mi355_group_destroy": (None, [vp]),
        "mi355_group_last_error": (C.c_char_p, [vp]),
        "mi355_group_submit_chain": (i, [vp, vp, u8p, u8p, i, i, i, i, C.POINTER(HsvSettings), C.POINTER(C.c_uint64)]),
        "mi355_group_submit_fused": (i, [vp, vp, u8p, u8p, i, i, i, i, C.POINTER(HsvSettings), C.POINTER(C.c_uint64)]),
        "mi355_group_flush": (i, [vp]),
        "mi355_pipe_set_group": (i, [vp, vp]),
        "mi355_group_wait": (i, [vp, C.c_uint64]),
        "mi355_group_order_after": (i, [vp, vp, C.c_uint64]),
        "mi355_group_wait_all": (i, [vp]),
        "mi355_group_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "mi355_group_set_rendezvous": (i, [vp, i, C.c_uint]),
        "mi355_group_set_compare_lanes": (i, [vp, i]),
        "mi355_group_submit_compare": (i, [vp, vp, u8p, u8p, i, i, i, i, i, C.POINTER(C.c_uint64)]),
        "mi355_group_wait_compare": (i, [vp, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
        "mi355_group_compare_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "mi355_group_set_colordetect_rendezvous": (i, [vp, i, C.c_uint]),
        "mi355_group_submit_colordetect": (i, [vp, vp, vp, sz, i, i, i, C.POINTER(C.c_uint64)]),
        "mi355_group_wait_colordetect": (i, [vp, C.c_uint64, u8p, C.POINTER(C.c_int)]),
        "mi355_group_colordetect_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "mi355_selftest_colordetect_plan": (i, [i, i, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                                C.POINTER(C.c_uint32)]),
        "mi355_group_set_hsvdetect_rendezvous": (i, [vp, i, C.c_uint]),
        "mi355_group_submit_hsvdetect": (i, [vp, vp, u8p, i, i, u8p, i, i, i, i, C.POINTER(HsvDetectSettings), C.POINTER(C.c_uint64)]),
        "mi355_group_wait_hsvdetect": (i, [vp, C.c_uint64]),
        "mi355_group_hsvdetect_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "mi355_selftest_hsvdetect_plan": (i, [i, i, C.c_uint, i, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                              C.POINTER(C.c_uint32)]),
        "mi355_group_set_hsvfilter_rendezvous": (i, [vp, i, C.c_uint]),
        "mi355_group_submit_hsvfilter": (i, [vp, vp, u8p, i, i, i, i, C.POINTER(HsvSettings), C.POINTER(C.c_uint64)]),
        "mi355_group_wait_hsvfilter": (i, [vp, C.c_uint64]),
        "mi355_group_hsvfilter_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "mi355_selftest_hsvfilter_set_plan": (i, [i, C.POINTER(HsvFilterPlanFrame), i, C.POINTER(HsvFilterPlanOut), C.POINTER(C.c_int)]),
        "mi355_group_set_colorlut_rendezvous": (i, [vp, i, C.c_uint]),
        "mi355_group_submit_colorlut": (i, [vp, vp, u8p, i, u8p, i, i, i, i, C.POINTER(C.c_uint64)]),
        "mi355_group_wait_colorlut": (i, [vp, C.c_uint64]),
        "mi355_group_colorlut_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "mi355_selftest_colorlut_set_plan": (i, [i, C.POINTER(ColorLutPlanFrame), i, C.POINTER(ColorLutPlanOut), C.POINTER(C.c_int)]),
        "mi355_agroup_create_echo": (vp, [i, i, sz, C.POINTER(C.c_int)]),
        "mi355_agroup_create_ebur128": (vp, [i, i, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mi355_agroup_create_loudnorm": (vp, [i, i, C.c_uint, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int)]),
        "mi355_agroup_destroy": (None, [vp]),
        "mi355_agroup_last_error": (C.c_char_p, [vp]),
        "mi355_agroup_set_linger": (i, [vp, C.c_uint, C.c_uint]),
        "mi355_agroup_detach": (i, [vp, i]),
        "mi355_agroup_submit_echo": (i, [vp, i, vp, sz, i, sz, C.c_double, C.c_double, i, C.POINTER(C.c_uint64)]),
        "mi355_agroup_submit_ebur128": (i, [vp, i, vp, sz, i, i, C.POINTER(C.c_uint64)]),
        "mi355_agroup_ebur128_reset": (i, [vp, i]),
        "mi355_agroup_submit_loudnorm": (i, [vp, i, vp, sz, vp, sz, i, i, C.POINTER(C.c_uint64)]),
        "mi355_agroup_loudnorm_frame_size": (sz, [vp, i]),
        "mi355_agroup_wait": (i, [vp, C.c_uint64, C.POINTER(sz)]),
        "mi355_agroup_ebur128_loudness": (i, [vp, i, i, C.POINTER(C.c_double)]),
        "mi355_agroup_ebur128_peak": (i, [vp, i, i, C.c_uint, C.POINTER(C.c_double)]),
        "mi355_agroup_echo_get_state": (i, [vp, i, vp, sz, C.POINTER(sz)]),
        "mi355_agroup_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "mi355_agroup_loudnorm_push": (i, [vp, i, vp, sz, vp, sz, C.POINTER(sz)]),
        "mi355_agroup_loudnorm_drain": (i, [vp, i, vp, sz, C.POINTER(sz), C.POINTER(C.c_int)]),
        "mi355_agroup_shared_echo": (vp, [i, i, sz, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mi355_agingradio_setup": (i, [vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint64]),
        "mi355_agingradio_process": (i, [vp, vp, sz, i, C.POINTER(AgingRadioSettings)]),
        "mi355_agingradio_process_device": (i, [vp, vp, sz, i, C.POINTER(AgingRadioSettings)]),
        "mi355_agingradio_get_state": (i, [vp, C.POINTER(C.c_double), C.c_uint, C.POINTER(C.c_uint64)]),
        "mi355_agingradio_reset": (i, [vp]),
        "mi355_agroup_create_agingradio": (vp, [i, i, C.POINTER(C.c_int)]),
        "mi355_agroup_shared_agingradio": (vp, [i, i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mi355_agroup_agingradio_setup": (i, [vp, i, C.c_uint, C.c_uint, C.c_uint, C.c_uint64]),
        "mi355_agroup_submit_agingradio": (i, [vp, i, vp, sz, i, C.POINTER(AgingRadioSettings), i, C.POINTER(C.c_uint64)]),
        "mi355_agroup_agingradio_get_state": (i, [vp, i, C.POINTER(C.c_double), C.c_uint, C.POINTER(C.c_uint64)]),
        "mi355_mixer_setup": (i, [vp, C.c_uint, C.c_uint, vp]),
        "mi355_mixer_setup_minus1": (i, [vp, C.c_uint]),
        "mi355_mixer_process": (i, [vp, C.POINTER(MixerSegment), C.c_uint, C.POINTER(MixerOutput), C.c_uint, sz]),
        "mi355_mixer_process_device": (i, [vp, C.POINTER(MixerSegment), C.c_uint, C.POINTER(MixerOutput), C.c_uint, sz]),
        "mi355_mixer_reset": (i, [vp]),
        "mi355_yolodec_tensor": (i, [vp, vp, i, C.c_uint32, C.c_uint32, C.POINTER(YoloParams), vp, C.c_uint32, C.POINTER(C.c_uint32)]),
        "mi355_yolodec_tensors_device": (i, [vp, vp, sz, i, i, C.c_uint32, C.c_uint32, C.POINTER(YoloParams), vp, C.c_uint32, C.POINTER(C.c_uint32)]),
        "mi355_selftest_yolodec_check": (i, [sz, i, i, C.c_uint32, C.c_uint32]),
        "mi355_yolox_head_decode_device": (i, [vp, C.POINTER(YoloxLevel), i, i, C.c_uint32, vp, sz]),
        "mi355_yolox_head_dets_device": (i, [vp, C.POINTER(YoloxLevel), i, i, C.c_uint32, C.POINTER(YoloParams), vp, C.c_uint32, C.POINTER(C.c_uint32)]),
        "mi355_yolox_head_dets": (i, [vp, C.POINTER(YoloxLevel), i, C.c_uint32, C.POINTER(YoloParams), vp, C.c_uint32, C.POINTER(C.c_uint32)]),
        "mi355_yolox_input_frames_device": (i, [vp, vp, sz, sz, i, C.c_uint32, C.c_uint32, vp, sz]),
        "mi355_selftest_yolox_head_check": (i, [C.POINTER(YoloxLevel), i, i, C.c_uint32, sz]),
        "mi355_yolox_net_create": (i, [vp, C.POINTER(YoloxNetConfig), C.POINTER(vp)]),
        "mi355_yolox_net_destroy": (None, [vp]),
        "mi355_yolox_net_param_count": (i, [vp]),
        "mi355_yolox_net_param_info": (i, [vp, i, C.c_char_p, sz, C.POINTER(C.c_uint32), C.POINTER(i)]),
        "mi355_yolox_net_set_param": (i, [vp, i, vp, sz]),
        "mi355_yolox_net_finalize": (i, [vp]),
        "mi355_yolox_net_forward_device": (i, [vp, vp, sz, i, C.c_uint32, C.c_uint32, C.POINTER(YoloxLevel)]),
        "mi355_yolox_net_launches": (i, [vp]),
        "mi355_yolox_net_arena_info": (i, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "mi355_yolox_infer_frames_device": (i, [vp, vp, sz, sz, i, C.c_uint32, C.c_uint32, vp, sz]),
        "mi355_yolox_infer_dets_device": (i, [vp, vp, sz, sz, i, C.c_uint32, C.c_uint32, C.POINTER(YoloParams), vp, C.c_uint32, C.POINTER(C.c_uint32)]),
        "mi355_selftest_yolox_net_plan": (i, [C.POINTER(YoloxNetConfig), i, C.c_uint32, C.c_uint32, C.POINTER(YoloxNetPlan)]),
        "mi355_selftest_yolox_net_param_info": (i, [C.POINTER(YoloxNetConfig), i, C.c_char_p, sz, C.POINTER(C.c_uint32), C.POINTER(i)]),
        "mi355_selftest_yolox_net_op_device": (i, [vp, C.POINTER(YoloxNetOp)]),
        "mi355_yolox_net_set_precision": (i, [vp, i]),
        "mi355_yolox_net_precision": (i, [vp]),
        "mi355_selftest_yolox_net_op_bf16_device": (i, [vp, C.POINTER(YoloxNetOp)]),
        "mi355_handdec_palm_tensor": (i, [vp, vp, C.c_uint32, C.POINTER(HandParams), vp, C.POINTER(C.c_uint32)]),
        "mi355_handdec_palm_tensors_device": (i, [vp, vp, sz, i, C.c_uint32, C.POINTER(HandParams), vp, C.POINTER(C.c_uint32)]),
        "mi355_handdec_landmarks_tensor": (i, [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.POINTER(HandParams), vp, vp, C.POINTER(C.c_uint32)]),
        "mi355_handdec_landmarks_tensors_device": (i, [vp, vp, sz, i, C.c_uint32, C.c_uint32, vp, sz, C.c_uint32, C.POINTER(HandParams), vp, vp,
                                                       C.POINTER(C.c_uint32)]),
        "mi355_selftest_handdec_check": (i, [i, sz, i, C.c_uint32, C.c_uint32, sz, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32]),
        "mi355_group_set_yolodec_rendezvous": (i, [vp, i, C.c_uint]),
        "mi355_group_submit_yolodec": (i, [vp, vp, vp, i, C.c_uint32, C.c_uint32, C.POINTER(YoloParams), C.c_uint32, C.POINTER(C.c_uint64)]),
        "mi355_group_wait_yolodec": (i, [vp, C.c_uint64, vp, C.POINTER(C.c_uint32)]),
        "mi355_group_yolodec_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "mi355_selftest_yolodec_set_plan": (i, [i, C.POINTER(C.c_int)] + [C.POINTER(C.c_uint32)] * 5 + [C.POINTER(C.c_uint64)] * 4),
        "mi355_group_submit_yolox_head": (i, [vp, vp, C.POINTER(YoloxLevel), i, C.c_uint32, C.POINTER(YoloParams), C.c_uint32, C.POINTER(C.c_uint64)]),
        "mi355_group_yolox_head_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "mi355_selftest_yolox_head_set_plan": (i, [i, C.POINTER(C.c_int)] + [C.POINTER(C.c_uint32)] * 3 + [C.POINTER(C.c_int)] + [C.POINTER(C.c_uint32)] * 5 +
                                               [C.POINTER(C.c_uint64)] * 3 + [C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
        "mi355_group_submit_yolox_infer": (i, [vp, vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.POINTER(YoloParams), C.c_uint32, C.POINTER(C.c_uint64)]),
        "mi355_group_release_yolox_net": (i, [vp, vp]),
        "mi355_group_yolox_infer_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "mi355_selftest_yolox_infer_set_plan": (i, [i, C.POINTER(C.c_int), C.POINTER(C.c_uint64)] + [C.POINTER(C.c_uint32)] * 2 + [C.POINTER(C.c_int32)] +
                                                [C.POINTER(C.c_uint32)] * 4 + [C.POINTER(C.c_uint64)]),
        "mi355_group_set_handdec_rendezvous": (i, [vp, i, C.c_uint]),
        "mi355_group_submit_handdec_palm": (i, [vp, vp, vp, C.c_uint32, C.POINTER(HandParams), C.POINTER(C.c_uint64)]),
        "mi355_group_submit_handdec_landmarks": (i, [vp, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.POINTER(HandParams), C.POINTER(C.c_uint64)]),
        "mi355_group_wait_handdec": (i, [vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint32)]),
        "mi355_group_handdec_stats": (i, [vp, C.POINTER(C.c_uint64)]),
        "mi355_selftest_handdec_set_plan": (i, [i, C.POINTER(C.c_int)] + [C.POINTER(C.c_uint32)] * 3 + [C.POINTER(C.c_uint64)]),
        "mi355_selftest_mixer_plan": (i, [i] + [C.POINTER(C.c_uint32)] * 4 + [C.POINTER(C.c_uint64)] + [C.POINTER(C.c_uint32)] * 4 + [C.c_uint32]
                                      + [C.POINTER(C.c_uint32)] * 3),
        "mi355_agroup_create_mixer": (vp, [i, i, C.POINTER(C.c_int)]),
        "mi355_agroup_shared_mixer": (vp, [i, i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mi355_agroup_mixer_setup": (i, [vp, i, C.c_uint, C.c_uint, vp]),
        "mi355_agroup_mixer_setup_minus1": (i, [vp, i, C.c_uint]),
        "mi355_agroup_submit_mixer": (i, [vp, i, C.POINTER(MixerSegment), C.c_uint, C.POINTER(MixerOutput), C.c_uint, sz, i, C.POINTER(C.c_uint64)]),
        "mi355_agroup_mixer_launches": (C.c_uint64, [vp]),
        "mi355_agroup_shared_ebur128": (vp, [i, i, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mi355_agroup_shared_loudnorm": (vp, [i, i, C.c_uint, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mi355_agroup_release": (None, [vp, i]),
        "mi355_group_shared": (vp, [i, C.POINTER(C.c_int)]),
        "mi355_group_release": (None, [vp]),
        "mi355_group_submit_round": (i, [vp, C.POINTER(vp), i, C.POINTER(vp), C.POINTER(vp), i, i, i, i, C.POINTER(HsvSettings)]),
        "mi355_group_submit_round_fused": (i, [vp, C.POINTER(vp), i, C.POINTER(vp), C.POINTER(vp), i, i, i, i, C.POINTER(HsvSettings)]),
        "mi355_dssim_compare_pairs": (i, [vp, C.POINTER(vp), C.POINTER(vp), i, i, i, i, i, C.POINTER(C.c_double)]),
        "mi355_dssim_compare_pairs_device": (i, [vp, C.POINTER(vp), C.POINTER(vp), i, i, i, i, i, C.POINTER(C.c_double)]),
        "mi355_dssim_pair_map_device": (i, [vp, vp, vp, i, i, i, i, i, f32p, C.POINTER(i), C.POINTER(i)]),
        "mi355_selftest_dssim_cbrt": (i, [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
        "mi355_selftest_dssim_plan": (i, [i, i, i, C.POINTER(DssimPlan)]),
        "mi355_selftest_dssim_compare_detail": (i, [vp, vp, vp, i, f32p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "mi355_dssim_image_plane": (i, [vp, vp, i, i, i, f32p, C.POINTER(i), C.POINTER(i)]),
        "mi355_sofa_setup": (i, [vp, i, i, i, i]),
        "mi355_sofa_set_filter": (i, [vp, i, f32p, f32p, i, i]),
        "mi355_sofa_set_drop": (i, [vp, i, i]),
        "mi355_sofa_reset": (i, [vp]),
        "mi355_sofa_teardown": (i, [vp]),
        "mi355_sofa_process_block": (i, [vp, f32p, f32p, f32p]),
        "mi355_sofa_process_block_device": (i, [vp, vp, vp, f32p]),
        "mi355_hrtf_load_sphere": (i, [vp, vp, sz, C.c_uint32]),
        "mi355_hrtf_setup": (i, [vp, i, i, i]),
        "mi355_hrtf_reset": (i, [vp]),
        "mi355_hrtf_teardown": (i, [vp]),
        "mi355_hrtf_process_block": (i, [vp, f32p, f32p, f32p, f32p]),
        "mi355_hrtf_process_block_device": (i, [vp, vp, vp, f32p, f32p]),
        "mi355_hrtf_sphere_info": (i, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "mi355_hrtf_transform_size": (i, [vp, C.POINTER(C.c_int)]),
        "mi355_hrtf_last_lookup": (i, [vp, C.POINTER(C.c_int), f32p]),
        "mi355_agroup_create_hrtf": (vp, [i, i, C.POINTER(C.c_int)]),
        "mi355_agroup_shared_hrtf": (vp, [i, i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mi355_agroup_hrtf_load_sphere": (i, [vp, i, vp, sz, C.c_uint32]),
        "mi355_agroup_hrtf_setup": (i, [vp, i, i, i, i, i]),
        "mi355_agroup_hrtf_reset": (i, [vp, i]),
        "mi355_agroup_submit_hrtf": (i, [vp, i, vp, vp, f32p, f32p, i, C.POINTER(C.c_uint64)]),
        "mi355_agroup_hrtf_info": (i, [vp, i, C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mi355_agroup_hrtf_last_lookup": (i, [vp, i, C.POINTER(C.c_int), f32p]),
        "mi355_agroup_hrtf_launches": (C.c_uint64, [vp]),
        "mi355_agroup_create_sofa": (vp, [i, i, C.POINTER(C.c_int)]),
        "mi355_agroup_shared_sofa": (vp, [i, i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mi355_agroup_sofa_setup": (i, [vp, i, i, i, i, i]),
        "mi355_agroup_sofa_set_filter": (i, [vp, i, i, f32p, f32p, i, i]),
        "mi355_agroup_sofa_set_drop": (i, [vp, i, i, i]),
        "mi355_agroup_sofa_reset": (i, [vp, i]),
        "mi355_agroup_submit_sofa": (i, [vp, i, vp, vp, i, f32p, i, C.POINTER(C.c_uint64)]),
        "mi355_agroup_sofa_info": (i, [vp, i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mi355_agroup_sofa_launches": (C.c_uint64, [vp]),
        "mi355_time_hsvfilter_device": (i, [vp, u8p, i, sz, i, i, i, i, C.POINTER(HsvSettings), i, f32p]),
        "mi355_time_hsv_colorlut_device": (i, [vp, u8p, sz, i, u8p, sz, i, i, i, i, C.POINTER(HsvSettings), i, f32p]),
        "mi355_time_colorlut_device": (i, [vp, u8p, sz, i, u8p, sz, i, i, i, i, i, i, f32p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


EXPORTED_SYMBOLS = None  # filled lazily by tests from the header


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a  # raw device pointer (int)


class StreamsRound:
    """n independent streams (one Context each) issued from one native loop per round: mi355_issue_streams_round. The pointer
    arrays are built once per (sources, destinations) pair so that a round costs one foreign call."""

    def __init__(self, contexts, width, height, stride, fmt, settings):
        self.L = load_library()
        self.n = len(contexts)
        self.ctxs = (C.c_void_p * self.n)(*[c.h for c in contexts])
        self.geom = (width, height, stride, FMT[fmt])
        self.settings = HsvSettings(*[float(v) for v in settings])
        self._arrays = {}

    def issue(self, src_ptrs, dst_ptrs):
        key = (tuple(src_ptrs), tuple(dst_ptrs))
        arr = self._arrays.get(key)
        if arr is None:
            arr = self._arrays[key] = ((C.c_void_p * self.n)(*src_ptrs), (C.c_void_p * self.n)(*dst_ptrs))
        rc = self.L.mi355_issue_streams_round(self.ctxs, self.n, arr[0], arr[1], *self.geom, C.byref(self.settings))
        if rc != 0:
            raise Mi355Error(rc, "mi355_issue_streams_round")


MAP_READ, MAP_WRITE = 1, 2


class DeviceBuffer:
    """mi355_buf: HBM + lazily created pinned shadow + dirty tracking (include/mi355fx.h "device buffers")."""

    def __init__(self, ctx, handle):
        self.ctx, self.L, self.h = ctx, ctx.L, handle

    @property
    def size(self):
        return int(self.L.mi355_buf_size(self.h))

    def device_ptr(self, ctx=None, flags=MAP_READ | MAP_WRITE):
        c = ctx or self.ctx
        p = self.L.mi355_buf_device_ptr(self.h, c.h, flags)
        if not p:
            raise Mi355Error(ERR_INVALID_ARG, (self.L.mi355_ctx_last_error(c.h) or b"").decode())
        return p

    def commit(self, ctx=None):
        (ctx or self.ctx)._ck(self.L.mi355_buf_commit(self.h, (ctx or self.ctx).h))

    def map(self, flags=MAP_READ):
        """numpy view of the pinned shadow (valid until unmap)."""
        p = self.L.mi355_buf_map_host(self.h, flags)
        if not p:
            raise Mi355Error(ERR_INVALID_ARG, (self.L.mi355_ctx_last_error(self.ctx.h) or b"").decode())
        return np.ctypeslib.as_array((C.c_uint8 * self.size).from_address(p))

    def unmap(self):
        self.ctx._ck(self.L.mi355_buf_unmap_host(self.h))

    def write(self, arr):
        v = self.map(MAP_WRITE)
        v[:] = np.ascontiguousarray(arr, dtype=np.uint8).reshape(-1)
        self.unmap()

    def read(self):
        v = self.map(MAP_READ).copy()
        self.unmap()
        return v

    def state(self):
        return self.L.mi355_buf_state(self.h)

    def close(self):
        if self.h:
            self.L.mi355_buf_unref(self.h)
            self.h = None


class Group:
    """Frames of many streams in few launches (mi355_group_*): submit_chain never blocks, wait(ticket) flushes if need be."""

    def __init__(self, device=0, max_batch=0):
        self.L = load_library()
        st = C.c_int(0)
        self.h = self.L.mi355_group_create(device, max_batch, C.byref(st))
        if not self.h:
            raise Mi355Error(st.value, "mi355_group_create")
        self._rounds = {}
        self._yolodec_caps = {}   # ticket -> the capacity its submit asked for (wait_yolodec sizes the result by it)
        self._handdec_landmarks = set()   # the landmark tickets (wait_handdec returns keypoint records for them)

    def _ck(self, rc):
        if rc != 0:
            raise Mi355Error(rc, (self.L.mi355_group_last_error(self.h) or b"").decode())

    def submit_chain(self, ctx, d_src, d_dst, width, height, stride, fmt, settings):
        s = HsvSettings(*[float(v) for v in settings])
        t = C.c_uint64(0)
        self._ck(self.L.mi355_group_submit_chain(self.h, ctx.h, d_src, d_dst, width, height, stride, FMT[fmt], C.byref(s), C.byref(t)))
        return t.value

    def submit_fused(self, ctx, d_src, d_dst, width, height, stride, fmt, settings):
        """The fused pair (source untouched) for one frame of one stream: ONE launch per batch through the composed table."""
        s = HsvSettings(*[float(v) for v in settings])
        t = C.c_uint64(0)
        self._ck(self.L.mi355_group_submit_fused(self.h, ctx.h, d_src, d_dst, width, height, stride, FMT[fmt], C.byref(s), C.byref(t)))
        return t.value

    def submit_round(self, contexts, src_ptrs, dst_ptrs, width, height, stride, fmt, settings, fused=False):
        """One frame of every stream from one native loop, then a flush (measurement plumbing)."""
        key = (tuple(c.h for c in contexts), tuple(src_ptrs), tuple(dst_ptrs))
        arr = self._rounds.get(key)
        if arr is None:
            n = len(contexts)
            arr = self._rounds[key] = ((C.c_void_p * n)(*[c.h for c in contexts]), (C.c_void_p * n)(*src_ptrs), (C.c_void_p * n)(*dst_ptrs))
        hs = HsvSettings(*[float(v) for v in settings])   # (only the pointer arrays are cached: the settings are this call's)
        fn = self.L.mi355_group_submit_round_fused if fused else self.L.mi355_group_submit_round
        self._ck(fn(self.h, arr[0], len(contexts), arr[1], arr[2], width, height, stride, FMT[fmt], C.byref(hs)))

    def flush(self):
        self._ck(self.L.mi355_group_flush(self.h))

    def wait(self, ticket):
        self._ck(self.L.mi355_group_wait(self.h, ticket))

    def order_after(self, ctx, ticket):
        """ctx's own stream waits (on the device) for that frame."""
        self._ck(self.L.mi355_group_order_after(self.h, ctx.h, ticket))

    def wait_all(self):
        self._ck(self.L.mi355_group_wait_all(self.h))

    def stats(self):
        """(frames, batched launch pairs, frames through their context's own path)."""
        c = (C.c_uint64 * 3)()
        self._ck(self.L.mi355_group_stats(self.h, c))
        return int(c[0]), int(c[1]), int(c[2])

    # ---- videocompare pairs of independent elements (Dssim / Blockhash)
    def set_rendezvous(self, expected_streams, linger_us):
        self._ck(self.L.mi355_group_set_rendezvous(self.h, expected_streams, linger_us))

    def set_compare_lanes(self, lanes):
        self._ck(self.L.mi355_group_set_compare_lanes(self.h, lanes))

    def submit_compare(self, ctx, d_ref, d_frame, stride, width, height, fmt="RGBA", algo=5):
        """One (reference frame, frame) pair of stream `ctx`; algo 5 = Dssim, 4 = Blockhash (mi355_hash_algo)."""
        t = C.c_uint64(0)
        self._ck(self.L.mi355_group_submit_compare(self.h, ctx.h, d_ref, d_frame, stride, width, height, FMT[fmt], algo, C.byref(t)))
        return t.value

    def wait_compare(self, ticket):
        """(distance, reference hash, frame hash): the dssim value / the Hamming distance and the two Blockhash hashes."""
        d = C.c_double(0.0)
        h = (C.c_uint64 * 2)()
        self._ck(self.L.mi355_group_wait_compare(self.h, ticket, C.byref(d), h))
        return d.value, int(h[0]), int(h[1])

    def compare_stats(self):
        """(pairs launched, launch sequences, pairs in the largest one)."""
        c = (C.c_uint64 * 3)()
        self._ck(self.L.mi355_group_compare_stats(self.h, c))
        return int(c[0]), int(c[1]), int(c[2])

    # ---- colordetect frames of independent elements
    def set_colordetect_rendezvous(self, expected_streams, linger_us):
        self._ck(self.L.mi355_group_set_colordetect_rendezvous(self.h, expected_streams, linger_us))

    def submit_colordetect(self, ctx, d_data, data_len, fmt, quality=10, max_colors=2):
        """One flat device plane of stream `ctx` (plane_data(0): strides ignored); returns the ticket."""
        t = C.c_uint64(0)
        self._ck(self.L.mi355_group_submit_colordetect(self.h, ctx.h, d_data, data_len, FMT[fmt], quality, max_colors, C.byref(t)))
        return t.value

    def wait_colordetect(self, ticket):
        """The frame's palette: a list of (r, g, b) in palette order, as Context.colordetect_frames_device returns per frame."""
        pal = np.zeros(255 * 3, np.uint8)
        n = C.c_int(0)
        self._ck(self.L.mi355_group_wait_colordetect(self.h, ticket, pal.ctypes.data, C.byref(n)))
        return [tuple(int(v) for v in pal[3 * k: 3 * k + 3]) for k in range(n.value)]

    def colordetect_stats(self):
        """(frames launched, launch sets, frames in the largest set, kernel launches)."""
        c = (C.c_uint64 * 4)()
        self._ck(self.L.mi355_group_colordetect_stats(self.h, c))
        return int(c[0]), int(c[1]), int(c[2]), int(c[3])

    # ---- hsvdetector frames of independent elements
    def set_hsvdetect_rendezvous(self, expected_streams, linger_us):
        self._ck(self.L.mi355_group_set_hsvdetect_rendezvous(self.h, expected_streams, linger_us))

    def submit_hsvdetect(self, ctx, d_src, src_stride, src_fmt, d_dst, dst_stride, dst_fmt, width, height, settings):
        """One device frame of stream `ctx` (settings: the six floats, or None for a null pointer); returns the ticket."""
        s = None if settings is None else C.byref(HsvDetectSettings(*[float(v) for v in settings]))
        t = C.c_uint64(0)
        self._ck(self.L.mi355_group_submit_hsvdetect(self.h, ctx.h, d_src, src_stride, FMT[src_fmt], d_dst, dst_stride, FMT[dst_fmt], width, height, s,
                                                     C.byref(t)))
        return t.value

    def wait_hsvdetect(self, ticket):
        """Returns once the frame's destination holds what Context.hsvdetect_frames_device would have written."""
        self._ck(self.L.mi355_group_wait_hsvdetect(self.h, ticket))

    def hsvdetect_stats(self):
        """(frames launched, launch sets, frames in the largest set, kernel launches)."""
        c = (C.c_uint64 * 4)()
        self._ck(self.L.mi355_group_hsvdetect_stats(self.h, c))
        return int(c[0]), int(c[1]), int(c[2]), int(c[3])

    # ---- hsvfilter frames of independent elements, in place
    def set_hsvfilter_rendezvous(self, expected_streams, linger_us):
        self._ck(self.L.mi355_group_set_hsvfilter_rendezvous(self.h, expected_streams, linger_us))

    def submit_hsvfilter(self, ctx, d_data, width, height, stride, fmt, settings):
        """One device frame of stream `ctx`, filtered in place (settings: the five floats, or None for a null pointer; fmt: a name
        or the enum's int); returns the ticket."""
        s = None if settings is None else C.byref(HsvSettings(*[float(v) for v in settings]))
        t = C.c_uint64(0)
        self._ck(self.L.mi355_group_submit_hsvfilter(self.h, ctx.h, d_data, width, height, stride, FMT.get(fmt, fmt), s, C.byref(t)))
        return t.value

    def wait_hsvfilter(self, ticket):
        """Returns once the frame holds what Context.hsvfilter_frames_device would have left."""
        self._ck(self.L.mi355_group_wait_hsvfilter(self.h, ticket))

    def hsvfilter_stats(self):
        """(frames launched, launch sets, frames in the largest set, kernel launches)."""
        c = (C.c_uint64 * 4)()
        self._ck(self.L.mi355_group_hsvfilter_stats(self.h, c))
        return int(c[0]), int(c[1]), int(c[2]), int(c[3])

    # ---- colorlut frames of independent elements, each through its context's LUT
    def set_colorlut_rendezvous(self, expected_streams, linger_us):
        self._ck(self.L.mi355_group_set_colorlut_rendezvous(self.h, expected_streams, linger_us))

    def submit_colorlut(self, ctx, d_src, src_stride, d_dst, dst_stride, width, height, fmt):
        """One device frame of stream `ctx`, source to destination through the LUT loaded in `ctx` (borrowed until the wait returns;
        fmt: a name or the enum's int); returns the ticket."""
        t = C.c_uint64(0)
        self._ck(self.L.mi355_group_submit_colorlut(self.h, ctx.h, d_src, src_stride, d_dst, dst_stride, width, height, FMT.get(fmt, fmt), C.byref(t)))
        return t.value

    def wait_colorlut(self, ticket):
        """Returns once the frame's destination holds what Context.colorlut_frames_device would have written."""
        self._ck(self.L.mi355_group_wait_colorlut(self.h, ticket))

    def colorlut_stats(self):
        """(frames launched, launch sets, frames in the largest set, kernel launches)."""
        c = (C.c_uint64 * 4)()
        self._ck(self.L.mi355_group_colorlut_stats(self.h, c))
        return int(c[0]), int(c[1]), int(c[2]), int(c[3])

    # ---- yolov8tensordec2 / yoloxtensordec tensors of independent elements
    def set_yolodec_rendezvous(self, expected_streams, linger_us):
        self._ck(self.L.mi355_group_set_yolodec_rendezvous(self.h, expected_streams, linger_us))

    def submit_yolodec(self, ctx, d_tensor, layout, num_fields, num_candidates, params, max_dets=None):
        """One device tensor of stream `ctx` (layout "V8": [F, N], "X": [N, F]; params: (box_thr, class_thr, iou_thr), a YoloParams, or
        None for a null pointer; max_dets: the capacity of the result, default N); returns the ticket."""
        cap = num_candidates if max_dets is None else max_dets
        p = None if params is None else _yolo_params(params)[0]
        t = C.c_uint64(0)
        self._ck(self.L.mi355_group_submit_yolodec(self.h, None if ctx is None else ctx.h, d_tensor, YOLO_LAYOUT.get(layout, layout), num_fields, num_candidates, p,
                                                   cap, C.byref(t)))
        self._yolodec_caps[t.value] = cap
        return t.value

    def wait_yolodec(self, ticket):
        """(records, count): the tensor's kept boxes as a YOLO_DET record array - the first min(count, max_dets) - and the full kept
        count, as Context.yolodec_device returns them for one tensor."""
        caps = self._yolodec_caps
        cap = caps.get(ticket, 0)
        dets = np.zeros(max(cap, 1), YOLO_DET)
        n = C.c_uint32(0)
        self._ck(self.L.mi355_group_wait_yolodec(self.h, ticket, dets.ctypes.data if cap else None, C.byref(n)))
        caps.pop(ticket, None)
        return dets[:min(n.value, cap)].copy(), n.value

    def yolodec_stats(self):
        """(tensors launched, launch sets, tensors in the largest set, kernel launches); a head counts as a tensor."""
        c = (C.c_uint64 * 4)()
        self._ck(self.L.mi355_group_yolodec_stats(self.h, c))
        return int(c[0]), int(c[1]), int(c[2]), int(c[3])

    def submit_yolox_head(self, ctx, levels, num_classes, params, max_dets=None, n_levels=None):
        """The raw head maps of one tensor of stream `ctx` as a member of the decoder queue (levels: as Context.yolox_head_dets_device
        takes them, or None for a null pointer; the pitches are ignored; max_dets: default A); returns the ticket, which
        wait_yolodec collects."""
        n = (0 if levels is None else len(levels)) if n_levels is None else n_levels
        cap = (0 if levels is None else yolox_candidates(levels)) if max_dets is None else max_dets
        p = None if params is None else _yolo_params(params)[0]
        t = C.c_uint64(0)
        self._ck(self.L.mi355_group_submit_yolox_head(self.h, None if ctx is None else ctx.h, None if levels is None else _yolox_levels(levels), n, num_classes, p, cap,
                                                      C.byref(t)))
        self._yolodec_caps[t.value] = cap
        return t.value

    def yolox_head_stats(self):
        """(heads launched, launch sets that held a head, level-table uploads, head kernel launches)."""
        c = (C.c_uint64 * 4)()
        self._ck(self.L.mi355_group_yolox_head_stats(self.h, c))
        return int(c[0]), int(c[1]), int(c[2]), int(c[3])

    def submit_yolox_infer(self, ctx, net, d_frame, stride, width, height, params, max_dets=None):
        """One RGB device frame of stream `ctx` for the finalized YoloxNet `net` as a member of the decoder queue (net: a YoloxNet, a
        raw handle, or None for a null pointer; params: (box_thr, class_thr, iou_thr), a YoloParams, or None for a null pointer;
        max_dets: default A of the frame size); returns the ticket, which wait_yolodec collects."""
        cap = sum((height >> (3 + l)) * (width >> (3 + l)) for l in range(3)) if max_dets is None else max_dets
        p = None if params is None else _yolo_params(params)[0]
        t = C.c_uint64(0)
        self._ck(self.L.mi355_group_submit_yolox_infer(self.h, None if ctx is None else ctx.h, getattr(net, "h", net), d_frame, stride, width, height, p, cap,
                                                       C.byref(t)))
        self._yolodec_caps[t.value] = cap
        return t.value

    def release_yolox_net(self, net):
        """Frees the queue's activation lanes of `net`; refused while a ticket that names it is pending or uncollected."""
        self._ck(self.L.mi355_group_release_yolox_net(self.h, getattr(net, "h", net)))

    def yolox_infer_stats(self):
        """(frames launched, forwards launched, frames in the largest forward, kernel launches of conversions and forwards, lanes
        alive, device allocations made for lanes since create)."""
        c = (C.c_uint64 * 6)()
        self._ck(self.L.mi355_group_yolox_infer_stats(self.h, c))
        return tuple(int(v) for v in c)

    # ---- handdetectiontensordec / handlandmarktensordec tensors of independent elements
    def set_handdec_rendezvous(self, expected_streams, linger_us):
        self._ck(self.L.mi355_group_set_handdec_rendezvous(self.h, expected_streams, linger_us))

    def submit_handdec_palm(self, ctx, d_tensor, num_rows, params):
        """One device palm tensor ([num_rows, 8] float32) of stream `ctx`; params: (confidence_thr, nms_iou_thr, max_hands[, frame_width,
        frame_height]), a HandParams, or None for a null pointer; returns the ticket."""
        p = None if params is None else _hand_params(params)[0]
        t = C.c_uint64(0)
        self._ck(self.L.mi355_group_submit_handdec_palm(self.h, None if ctx is None else ctx.h, d_tensor, num_rows, p, C.byref(t)))
        return t.value

    def submit_handdec_landmarks(self, ctx, d_landmarks, num_hands, kps_dim, params, d_scores=None, num_scores=0):
        """One device landmark tensor ([num_hands, 21 * kps_dim] float32) of stream `ctx`, with its num_scores device scores or None;
        params as submit_handdec_palm; returns the ticket."""
        p = None if params is None else _hand_params(params)[0]
        t = C.c_uint64(0)
        self._ck(self.L.mi355_group_submit_handdec_landmarks(self.h, None if ctx is None else ctx.h, d_landmarks, num_hands, kps_dim, d_scores, num_scores, p,
                                                             C.byref(t)))
        self._handdec_landmarks.add(t.value)
        return t.value

    def wait_handdec(self, ticket):
        """The tensor's hands as Context.handdec_palm_device / handdec_landmarks_device return them for one tensor: a HAND_DET record
        array for a palm ticket, (HAND_DET records, HAND_KP records) for a landmark ticket."""
        landmarks = ticket in self._handdec_landmarks
        dets, kps = np.zeros(HAND_MAX, HAND_DET), np.zeros(HAND_MAX, HAND_KP)
        n = C.c_uint32(0)
        self._ck(self.L.mi355_group_wait_handdec(self.h, ticket, dets.ctypes.data, kps.ctypes.data, C.byref(n)))
        self._handdec_landmarks.discard(ticket)
        return (dets[:n.value].copy(), kps[:n.value].copy()) if landmarks else dets[:n.value].copy()

    def handdec_stats(self):
        """(tensors launched, launch sets, tensors in the largest set, kernel launches)."""
        c = (C.c_uint64 * 4)()
        self._ck(self.L.mi355_group_handdec_stats(self.h, c))
        return int(c[0]), int(c[1]), int(c[2]), int(c[3])

    def close(self):
        if self.h:
            self.L.mi355_group_destroy(self.h)
            self.h = None


def selftest_hsvfilter_set_plan(frames, n_cu=256):
    """mi355_selftest_hsvfilter_set_plan (host only): what the hsvfilter queue's builder makes of frames in submission order.
    frames: (address, width, height, stride, fmt, settings[, force_generic]) each, the address a number that is never dereferenced,
    fmt a name or the enum's int; or None for null arrays. Returns (status, n_sets, [dict(set, launch, variant, units, first_block,
    blocks)])."""
    L = load_library()
    n_sets = C.c_int(-1)
    if frames is None:
        return L.mi355_selftest_hsvfilter_set_plan(n_cu, None, 1, None, C.byref(n_sets)), n_sets.value, []
    n = len(frames)
    m = max(n, 1)
    fr, out = (HsvFilterPlanFrame * m)(), (HsvFilterPlanOut * m)()
    for k, f in enumerate(frames):
        fr[k] = HsvFilterPlanFrame(f[0], f[1], f[2], f[3], FMT.get(f[4], f[4]), HsvSettings(*[float(v) for v in f[5]]), int(f[6]) if len(f) > 6 else 0)
    rc = L.mi355_selftest_hsvfilter_set_plan(n_cu, fr, n, out, C.byref(n_sets))
    return rc, n_sets.value, [dict(set=o.set, launch=o.launch, variant=o.variant, units=int(o.units), first_block=o.first_block, blocks=o.blocks)
                              for o in list(out)[:n]]


def selftest_colorlut_set_plan(frames, n_cu=256):
    """mi355_selftest_colorlut_set_plan (host only): what the colorlut queue's builder makes of frames in submission order.
    frames: (src_address, src_stride, dst_address, dst_stride, width, height, fmt[, force_generic]) each, the addresses numbers that
    are never dereferenced, fmt a name or the enum's int; or None for null arrays. Returns (status, n_sets, [dict(set, launch,
    geometry, units, first_block, blocks)])."""
    L = load_library()
    n_sets = C.c_int(-1)
    if frames is None:
        return L.mi355_selftest_colorlut_set_plan(n_cu, None, 1, None, C.byref(n_sets)), n_sets.value, []
    n = len(frames)
    m = max(n, 1)
    fr, out = (ColorLutPlanFrame * m)(), (ColorLutPlanOut * m)()
    for k, f in enumerate(frames):
        fr[k] = ColorLutPlanFrame(f[0], f[2], f[1], f[3], f[4], f[5], FMT.get(f[6], f[6]), int(f[7]) if len(f) > 7 else 0)
    rc = L.mi355_selftest_colorlut_set_plan(n_cu, fr, n, out, C.byref(n_sets))
    return rc, n_sets.value, [dict(set=o.set, launch=o.launch, geometry=o.geometry, units=int(o.units), first_block=o.first_block, blocks=o.blocks)
                              for o in list(out)[:n]]


def selftest_dssim_plan(width, height, n_cu=256):
    """mi355_selftest_dssim_plan (host only): the exact Dssim engine's geometry of a width x height frame on n_cu compute units.
    Returns (status, dict): tile = (tile_w, tile_h, tile_lanes, scale_halo, compare_halo); scales = [(w, h)]; tiles, interior_scale,
    interior_compare, downsample_blocks, absdev_blocks per scale; launches = [(first scale, jobs, first[0..3])]; avg_blocks,
    sum_blocks. The dict is None when the status is not 0."""
    L = load_library()
    p = DssimPlan()
    rc = L.mi355_selftest_dssim_plan(width, height, n_cu, C.byref(p))
    if rc:
        return rc, None
    ns = p.n_scales
    return rc, dict(tile=(p.tile_w, p.tile_h, p.tile_lanes, p.scale_halo, p.compare_halo), scales=[(p.w[k], p.h[k]) for k in range(ns)],
                    tiles=list(p.tiles)[:ns], interior_scale=list(p.interior_scale)[:ns], interior_compare=list(p.interior_compare)[:ns],
                    downsample_blocks=list(p.downsample_blocks)[:ns], absdev_blocks=list(p.absdev_blocks)[:ns],
                    launches=[(p.launch_scale[l], p.launch_jobs[l], tuple(p.launch_first[l])) for l in range(p.n_launches)],
                    avg_blocks=p.avg_blocks, sum_blocks=p.sum_blocks)


def selftest_handdec_set_plan(decoders, rows):
    """mi355_selftest_handdec_set_plan (host only): the layout of one hand-decoder launch set. Returns (status, block, kp_slot,
    totals); decoders: 0 (palm) / 1 (landmarks) per job."""
    L = load_library()
    n = len(decoders)
    m = max(n, 1)
    dec, r = (C.c_int * m)(*decoders), (C.c_uint32 * m)(*rows)
    block, kp_slot, totals = (C.c_uint32 * m)(), (C.c_uint32 * m)(), (C.c_uint64 * 4)()
    rc = L.mi355_selftest_handdec_set_plan(n, dec, r, block, kp_slot, totals)
    return rc, list(block)[:n], list(kp_slot)[:n], list(totals)


def selftest_yolox_head_check(levels, n_tensors, num_classes, out_pitch_bytes, n_levels=None):
    """mi355_selftest_yolox_head_check (host only): the status the shape checks of the YOLOX head entry points give. levels: as
    Context.yolox_head_decode_device takes them, or None; the pointers are never dereferenced. n_levels: default len(levels)."""
    L = load_library()
    n = (0 if levels is None else len(levels)) if n_levels is None else n_levels
    return L.mi355_selftest_yolox_head_check(None if levels is None else _yolox_levels(levels), n, n_tensors, num_classes, out_pitch_bytes)


def _yolox_param_table(fn, n=None):
    """[(name, dims)] of a parameter enumeration: fn(index, name buffer, cap, dims, n_dims) -> status; n None: until the first refusal."""
    out, k = [], 0
    name, dims, nd = C.create_string_buffer(YOLOX_NET_NAME_MAX), (C.c_uint32 * 4)(), C.c_int(0)
    while n is None or k < n:
        rc = fn(k, name, YOLOX_NET_NAME_MAX, dims, C.byref(nd))
        if rc != 0:
            if n is None:
                break
            raise Mi355Error(rc, "yolox_net parameter %d" % k)
        out.append((name.value.decode(), tuple(int(d) for d in dims[:nd.value])))
        k += 1
    return out


def selftest_yolox_net_plan(config, n_frames, H, W):
    """mi355_selftest_yolox_net_plan (host only) -> (status, YoloxNetPlan). config: a YoloxNetConfig or None."""
    L = load_library()
    plan = YoloxNetPlan()
    rc = L.mi355_selftest_yolox_net_plan(None if config is None else C.byref(config), n_frames, H, W, C.byref(plan))
    return rc, plan


def selftest_yolox_net_params(config, n=None):
    """The parameter table of a config without a device (mi355_selftest_yolox_net_param_info): [(name, dims)] in the net's order."""
    L = load_library()
    return _yolox_param_table(lambda k, name, cap, dims, nd: L.mi355_selftest_yolox_net_param_info(C.byref(config), k, name, cap, dims, nd), n)


class YoloxNet:
    """mi355_yolox_net: yoloxinference's network on one Context. Set every parameter (set_param / load), finalize(), then forward_device
    or the two compositions. Destroy it (close) before its context."""

    def __init__(self, ctx, config):
        self.ctx, self.L, self.config = ctx, ctx.L, config
        h = C.c_void_p()
        self.h = None
        ctx._ck(self.L.mi355_yolox_net_create(ctx.h, None if config is None else C.byref(config), C.byref(h)))
        self.h = h.value
        self.num_classes = int(config.num_classes)

    def close(self):
        if getattr(self, "h", None):
            self.L.mi355_yolox_net_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def param_count(self):
        return int(self.L.mi355_yolox_net_param_count(self.h))

    def params(self):
        return _yolox_param_table(lambda k, name, cap, dims, nd: self.L.mi355_yolox_net_param_info(self.h, k, name, cap, dims, nd), self.param_count())

    def set_param(self, index, values, n=None):
        a = np.ascontiguousarray(values, dtype=np.float32)
        self.ctx._ck(self.L.mi355_yolox_net_set_param(self.h, index, a.ctypes.data, a.size if n is None else n))

    def load(self, arrays):
        """arrays: {name: array} holding every parameter of params()."""
        for k, (name, dims) in enumerate(self.params()):
            self.set_param(k, np.asarray(arrays[name], dtype=np.float32).reshape(dims))

    def set_precision(self, precision):
        """mi355_yolox_net_set_precision: "f32" (the default) / "bf16" or the enum's ints; before finalize() only."""
        self.ctx._ck(self.L.mi355_yolox_net_set_precision(self.h, YOLOX_PRECISION.get(precision, precision)))

    def precision(self):
        return int(self.L.mi355_yolox_net_precision(self.h))

    def finalize(self):
        self.ctx._ck(self.L.mi355_yolox_net_finalize(self.h))

    def launches(self):
        return int(self.L.mi355_yolox_net_launches(self.h))

    def arena_info(self):
        """(arena bytes, device allocations made for activations so far)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.ctx._ck(self.L.mi355_yolox_net_arena_info(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def forward_device(self, d_in, in_pitch_bytes, n_frames, H, W):
        """-> the three YoloxLevel structs (device pointers into the net's memory, valid until the next forward). Asynchronous."""
        lv = (YoloxLevel * 3)()
        self.ctx._ck(self.L.mi355_yolox_net_forward_device(self.h, d_in, in_pitch_bytes, n_frames, H, W, lv))
        return [lv[0], lv[1], lv[2]]

    def read_levels(self, levels, n_frames):
        """The raw maps of forward_device's levels read back: per level an array [n_frames, 5 + C, h, w] (reg 0:4, obj 4, cls 5:)."""
        self.ctx.synchronize()
        out = []
        for lv in levels:
            a = np.empty((n_frames, 5 + self.num_classes, lv.h, lv.w), np.float32)
            assert lv.reg_pitch_bytes == a[0].nbytes and lv.obj == lv.reg + 16 * lv.h * lv.w and lv.cls == lv.reg + 20 * lv.h * lv.w
            self.ctx.d2h(a, lv.reg)
            out.append(a)
        return out

    def infer_frames_device(self, d_frames, frame_pitch, stride, n_frames, width, height, d_out, out_pitch_bytes):
        self.ctx._ck(self.L.mi355_yolox_infer_frames_device(self.h, d_frames, frame_pitch, stride, n_frames, width, height, d_out, out_pitch_bytes))

    def infer_dets_device(self, d_frames, frame_pitch, stride, n_frames, width, height, params, max_dets, return_counts=False):
        p, n_p = _yolo_params(params)
        if n_p != n_frames:
            raise ValueError("yolox infer_dets_device: one settings triple per frame")
        dets = np.zeros((n_frames, max(max_dets, 1)), YOLO_DET)
        n = (C.c_uint32 * n_frames)()
        self.ctx._ck(self.L.mi355_yolox_infer_dets_device(self.h, d_frames, frame_pitch, stride, n_frames, width, height, p, dets.ctypes.data, max_dets, n))
        out = [dets[k, :min(n[k], max_dets)].copy() for k in range(n_frames)]
        return (out, [int(v) for v in n]) if return_counts else out


def selftest_yolodec_set_plan(layouts, num_fields, num_candidates, max_dets):
    """mi355_selftest_yolodec_set_plan (host only): the layout of one decoder launch set. Returns (status, first_block, blocks,
    key_offset, box_offset, det_offset, totals); layouts: "V8" / "X" or the enum's ints."""
    L = load_library()
    n = len(layouts)
    m = max(n, 1)
    lay = (C.c_int * m)(*[YOLO_LAYOUT.get(v, v) for v in layouts])
    F, N, cap = (C.c_uint32 * m)(*num_fields), (C.c_uint32 * m)(*num_candidates), (C.c_uint32 * m)(*max_dets)
    first, blocks = (C.c_uint32 * m)(), (C.c_uint32 * m)()
    key, box, det, totals = (C.c_uint64 * m)(), (C.c_uint64 * m)(), (C.c_uint64 * m)(), (C.c_uint64 * 6)()
    rc = L.mi355_selftest_yolodec_set_plan(n, lay, F, N, cap, first, blocks, key, box, det, totals)
    return rc, list(first)[:n], list(blocks)[:n], list(key)[:n], list(box)[:n], list(det)[:n], list(totals)


def selftest_yolox_head_set_plan(kinds, num_fields, num_candidates, max_dets, level_shapes):
    """mi355_selftest_yolox_head_set_plan (host only): the layout of one decoder launch set that may hold heads. kinds: "V8" / "X" /
    YOLO_X_HEAD or ints; level_shapes: per job a list of (h, w) - a head job's levels, anything empty for a tensor job - or None for
    null level arrays. Returns (status, candidates, first_block, blocks, key_offset, box_offset, det_offset, level_first_block,
    totals); level_first_block is per job, as level_shapes is."""
    L = load_library()
    n = len(kinds)
    m = max(n, 1)
    kind = (C.c_int * m)(*[YOLO_LAYOUT.get(v, v) for v in kinds])
    F, N, cap = (C.c_uint32 * m)(*num_fields), (C.c_uint32 * m)(*num_candidates), (C.c_uint32 * m)(*max_dets)
    if level_shapes is None:
        nl = lh = lw = lfirst = None
        counts = [0] * n
    else:
        counts = [len(q) for q in level_shapes]
        flat = [hw for q in level_shapes for hw in q]
        k = max(len(flat), 1)
        nl = (C.c_int * m)(*counts)
        lh, lw, lfirst = (C.c_uint32 * k)(*[q[0] for q in flat]), (C.c_uint32 * k)(*[q[1] for q in flat]), (C.c_uint32 * k)()
    cand, first, blocks = (C.c_uint32 * m)(), (C.c_uint32 * m)(), (C.c_uint32 * m)()
    key, box, det, totals = (C.c_uint64 * m)(), (C.c_uint64 * m)(), (C.c_uint64 * m)(), (C.c_uint64 * 8)()
    rc = L.mi355_selftest_yolox_head_set_plan(n, kind, F, N, cap, nl, lh, lw, cand, first, blocks, key, box, det, lfirst, totals)
    per_job, at = [], 0
    for c in counts:
        per_job.append([] if lfirst is None else list(lfirst[at: at + c]))
        at += c
    return rc, list(cand)[:n], list(first)[:n], list(blocks)[:n], list(key)[:n], list(box)[:n], list(det)[:n], per_job, list(totals)


def selftest_yolox_infer_set_plan(kinds, net_keys, heights, widths, null=()):
    """mi355_selftest_yolox_infer_set_plan (host only): the infer side of one decoder launch set. kinds: "V8" / "X" / YOLO_X_HEAD /
    YOLO_X_INFER or ints; null: names of arguments passed as null pointers (kind, net_key, height, width, class_of, frame_in_class,
    conv_first_block, conv_blocks, class_frames, totals). Returns (status, class_of, frame_in_class, conv_first_block, conv_blocks,
    class_frames, totals); class_frames holds one entry per class."""
    L = load_library()
    n = len(kinds)
    m = max(n, 1)
    a = {"kind": (C.c_int * m)(*[YOLO_LAYOUT.get(v, v) for v in kinds]), "net_key": (C.c_uint64 * m)(*net_keys), "height": (C.c_uint32 * m)(*heights),
         "width": (C.c_uint32 * m)(*widths), "class_of": (C.c_int32 * m)(), "frame_in_class": (C.c_uint32 * m)(), "conv_first_block": (C.c_uint32 * m)(),
         "conv_blocks": (C.c_uint32 * m)(), "class_frames": (C.c_uint32 * m)(), "totals": (C.c_uint64 * 3)()}
    rc = L.mi355_selftest_yolox_infer_set_plan(n, *[None if k in null else v for k, v in a.items()])
    totals = list(a["totals"])
    return (rc, list(a["class_of"])[:n], list(a["frame_in_class"])[:n], list(a["conv_first_block"])[:n], list(a["conv_blocks"])[:n],
            list(a["class_frames"])[:int(totals[0]) if rc == 0 else 0], totals)


class AudioGroup:
    """Independent audio element instances of one kind and configuration sharing launches (mi355_agroup_*)."""

    def __init__(self, kind, n_members, device=0, shared=False, **kw):
        """shared=True: the process-wide group of this configuration (mi355_agroup_shared_*); self.member is the index handed out,
        close() releases the membership (the last member out destroys the group)."""
        self.L = load_library()
        st = C.c_int(0)
        self.kind, self.n = kind, n_members
        self.channels = kw.get("channels", 1)
        self.shared, self.member = shared, None
        if shared:
            m = C.c_int(-1)
            if kind == "echo":
                self.h = self.L.mi355_agroup_shared_echo(device, n_members, kw["ring_len"], C.byref(m), C.byref(st))
            elif kind == "agingradio":
                self.h = self.L.mi355_agroup_shared_agingradio(device, n_members, C.byref(m), C.byref(st))
            elif kind == "hrtf":
                self.h = self.L.mi355_agroup_shared_hrtf(device, n_members, C.byref(m), C.byref(st))
            elif kind == "sofa":
                self.h = self.L.mi355_agroup_shared_sofa(device, n_members, C.byref(m), C.byref(st))
            elif kind == "mixer":
                self.h = self.L.mi355_agroup_shared_mixer(device, n_members, C.byref(m), C.byref(st))
            elif kind == "ebur128":
                cc = kw.get("channel_class")
                arr = (C.c_int * len(cc))(*cc) if cc is not None else None
                self.h = self.L.mi355_agroup_shared_ebur128(device, n_members, kw["channels"], kw["rate"], kw["mode"], arr, C.byref(m), C.byref(st))
            else:
                self.h = self.L.mi355_agroup_shared_loudnorm(device, n_members, kw["channels"], kw.get("loudness_target", -24.0), kw.get("loudness_range_target", 7.0),
                                                             kw.get("max_true_peak", -2.0), kw.get("offset", 0.0), C.byref(m), C.byref(st))
            if not self.h:
                raise Mi355Error(st.value, "mi355_agroup_shared_" + kind)
            self.member = m.value
            self._keep = {}
            return
        if kind == "echo":
            self.h = self.L.mi355_agroup_create_echo(device, n_members, kw["ring_len"], C.byref(st))
        elif kind == "agingradio":
            self.h = self.L.mi355_agroup_create_agingradio(device, n_members, C.byref(st))
        elif kind == "hrtf":
            self.h = self.L.mi355_agroup_create_hrtf(device, n_members, C.byref(st))
        elif kind == "sofa":
            self.h = self.L.mi355_agroup_create_sofa(device, n_members, C.byref(st))
        elif kind == "mixer":
            self.h = self.L.mi355_agroup_create_mixer(device, n_members, C.byref(st))
        elif kind == "ebur128":
            cc = kw.get("channel_class")
            arr = (C.c_int * len(cc))(*cc) if cc is not None else None
            self.h = self.L.mi355_agroup_create_ebur128(device, n_members, kw["channels"], kw["rate"], kw["mode"], arr, C.byref(st))
            self.channels = kw["channels"]
        elif kind == "loudnorm":
            self.h = self.L.mi355_agroup_create_loudnorm(device, n_members, kw["channels"], kw.get("loudness_target", -24.0), kw.get("loudness_range_target", 7.0),
                                                         kw.get("max_true_peak", -2.0), kw.get("offset", 0.0), C.byref(st))
            self.channels = kw["channels"]
        else:
            raise ValueError(kind)
        if not self.h:
            raise Mi355Error(st.value, "mi355_agroup_create_" + kind)
        self._keep = {}

    def _ck(self, rc):
        if rc != 0:
            raise Mi355Error(rc, (self.L.mi355_agroup_last_error(self.h) or b"").decode())

    def set_linger(self, linger_us=0, timeout_ms=0):
        self._ck(self.L.mi355_agroup_set_linger(self.h, linger_us, timeout_ms))

    def detach(self, member):
        self._ck(self.L.mi355_agroup_detach(self.h, member))

    def submit_echo(self, member, data, delay, intensity, feedback, n=None, is_f64=None):
        """data: a numpy f32 / f64 array (host, processed in place and valid after wait) or a device pointer (then n, is_f64)."""
        t = C.c_uint64(0)
        if isinstance(data, np.ndarray):
            assert data.flags.c_contiguous and data.dtype in (np.float32, np.float64)
            self._ck(self.L.mi355_agroup_submit_echo(self.h, member, data.ctypes.data, data.size, int(data.dtype == np.float64), delay, intensity, feedback, 0, C.byref(t)))
            self._keep[member] = data     # (after the call: a refused submit must not drop the buffer an outstanding ticket still fills)
        else:
            self._ck(self.L.mi355_agroup_submit_echo(self.h, member, data, n, int(bool(is_f64)), delay, intensity, feedback, 1, C.byref(t)))
        return t.value

    def agingradio_setup(self, member, channels, rate, lowpass_freq, seed):
        """AudioFilterImpl::setup of one agingradio member: its filters, pair counter and seed start over."""
        self._ck(self.L.mi355_agroup_agingradio_setup(self.h, member, channels, rate, lowpass_freq, seed))

    def submit_agingradio(self, member, data, settings, channels=None, frames=None, is_f64=None):
        """data: a numpy f32 / f64 array of frames * channels (host, processed in place, valid after wait) or a device pointer
        (then frames, is_f64). settings: a dict of mi355_agingradio_settings fields (missing ones at the element's defaults)."""
        t = C.c_uint64(0)
        st = AgingRadioSettings.of(settings)
        if isinstance(data, np.ndarray):
            assert data.flags.c_contiguous and data.dtype in (np.float32, np.float64)
            self._ck(self.L.mi355_agroup_submit_agingradio(self.h, member, data.ctypes.data, data.size // channels, int(data.dtype == np.float64), C.byref(st), 0,
                                                           C.byref(t)))
            self._keep[member] = data
        else:
            self._ck(self.L.mi355_agroup_submit_agingradio(self.h, member, data, frames, int(bool(is_f64)), C.byref(st), 1, C.byref(t)))
        return t.value

    def agingradio_state(self, member, channels):
        y = np.zeros(max(channels, 1), np.float64)
        k = C.c_uint64(0)
        self._ck(self.L.mi355_agroup_agingradio_get_state(self.h, member, y.ctypes.data_as(C.POINTER(C.c_double)), channels, C.byref(k)))
        return y[:channels], int(k.value)

    # ---- hrtfrender members
    def hrtf_load_sphere(self, member, data, rate):
        """HrirSphere::new(bytes, rate) of one member; identical bytes at the same rate are kept once on the device"""
        b = bytes(data)
        buf = (C.c_uint8 * len(b)).from_buffer_copy(b)
        self._ck(self.L.mi355_agroup_hrtf_load_sphere(self.h, member, C.cast(buf, C.c_void_p), len(b), rate))

    def hrtf_setup(self, member, channels, block_length=512, interpolation_steps=8, method=0):
        """set_caps of one member; method as FLAG_HRTF_METHOD of a lone Context (0 by HRIR length, 1 FFT, 2 FIR)"""
        self._ck(self.L.mi355_agroup_hrtf_setup(self.h, member, channels, block_length, interpolation_steps, method))
        if not hasattr(self, "_hrtf_shape"):
            self._hrtf_shape = {}
        self._hrtf_shape[member] = (channels, block_length * interpolation_steps, interpolation_steps)

    def hrtf_reset(self, member):
        """State::reset_processors of one member: tails cleared, previous directions and gains kept"""
        self._ck(self.L.mi355_agroup_hrtf_reset(self.h, member))

    def submit_hrtf(self, member, inp, positions, gains, out=None):
        """One block. inp: numpy f32 [frames, channels] (host; -> ticket, and the f32 [frames * 2] output array is hrtf_output(member)
        once the ticket has been waited for) or a device pointer (then out: the device pointer of the output)."""
        channels, frames, _ = self._hrtf_shape[member]
        fp = C.POINTER(C.c_float)
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1)
        g = np.ascontiguousarray(gains, dtype=np.float32).reshape(-1)
        assert pos.size == 3 * channels and g.size == channels
        t = C.c_uint64(0)
        if isinstance(inp, np.ndarray):
            x = np.ascontiguousarray(inp, dtype=np.float32).reshape(-1)
            assert x.size == frames * channels, "one block = block_length*interpolation_steps frames"
            y = np.zeros(frames * 2, np.float32)
            self._ck(self.L.mi355_agroup_submit_hrtf(self.h, member, x.ctypes.data, y.ctypes.data, pos.ctypes.data_as(fp), g.ctypes.data_as(fp), 0, C.byref(t)))
            self._keep[member] = (x, y)   # (after the call: a refused submit leaves hrtf_output(member) the array the outstanding ticket fills)
        else:
            self._ck(self.L.mi355_agroup_submit_hrtf(self.h, member, inp, out, pos.ctypes.data_as(fp), g.ctypes.data_as(fp), 1, C.byref(t)))
        return t.value

    def hrtf_output(self, member):
        """the output array of the member's last host submission (filled by wait)"""
        return self._keep[member][1]

    def hrtf_info(self, member):
        """(HRIR length, transform size: 0 = FIR, -1 before setup, distinct spheres the group holds on the device)"""
        a, n, k = C.c_uint32(0), C.c_int(-1), C.c_int(0)
        self._ck(self.L.mi355_agroup_hrtf_info(self.h, member, C.byref(a), C.byref(n), C.byref(k)))
        return a.value, n.value, k.value

    def hrtf_last_lookup(self, member):
        channels, _, steps = self._hrtf_shape[member]
        faces = np.zeros(channels * steps, np.int32)
        uvw = np.zeros(channels * steps * 3, np.float32)
        self._ck(self.L.mi355_agroup_hrtf_last_lookup(self.h, member, faces.ctypes.data_as(C.POINTER(C.c_int)), uvw.ctypes.data_as(C.POINTER(C.c_float))))
        return faces.reshape(channels, steps), uvw.reshape(channels, steps, 3)

    def hrtf_launches(self):
        return int(self.L.mi355_agroup_hrtf_launches(self.h))

    # ---- sofalizer members
    def sofa_setup(self, member, channels, filter_len, partition_length=64, block_length=256):
        """set_caps of one member; the checks and messages of Context.sofa_setup"""
        self._ck(self.L.mi355_agroup_sofa_setup(self.h, member, channels, filter_len, partition_length, block_length))
        if not hasattr(self, "_sofa_shape"):
            self._sofa_shape = {}
        self._sofa_shape[member] = (channels, block_length)

    def sofa_set_filter(self, member, channel, left, right, delay_left=0, delay_right=0):
        """queued: copied now, transformed with the member's next launch set (a second call for the channel before that replaces it)"""
        fp = C.POINTER(C.c_float)
        l, r = np.ascontiguousarray(left, np.float32), np.ascontiguousarray(right, np.float32)
        self._ck(self.L.mi355_agroup_sofa_set_filter(self.h, member, channel, l.ctypes.data_as(fp), r.ctypes.data_as(fp), delay_left, delay_right))

    def sofa_set_drop(self, member, channel, drop=True):
        self._ck(self.L.mi355_agroup_sofa_set_drop(self.h, member, channel, int(drop)))

    def sofa_reset(self, member):
        """flush-stop of one member: history cleared, filters (transformed and pending) kept"""
        self._ck(self.L.mi355_agroup_sofa_reset(self.h, member))

    def submit_sofa(self, member, inp, gains, n_blocks=1, out=None):
        """n_blocks whole blocks. inp: numpy f32 [n_blocks * block_length, channels] (host; -> ticket, and the f32 [n_blocks * block_length, 2]
        output array is sofa_output(member) once the ticket has been waited for) or a device pointer (then out: the device pointer of the output)."""
        channels, block = self._sofa_shape[member]
        fp = C.POINTER(C.c_float)
        g = np.ascontiguousarray(gains, dtype=np.float32).reshape(-1)
        assert g.size == channels
        t = C.c_uint64(0)
        if isinstance(inp, np.ndarray):
            x = np.ascontiguousarray(inp, dtype=np.float32).reshape(-1)
            assert x.size == max(n_blocks, 0) * block * channels or not 1 <= n_blocks <= 8, "a buffer = n_blocks * block_length frames"
            y = np.zeros((max(n_blocks, 1) * block, 2), np.float32)
            self._ck(self.L.mi355_agroup_submit_sofa(self.h, member, x.ctypes.data, y.ctypes.data, n_blocks, g.ctypes.data_as(fp), 0, C.byref(t)))
            self._keep[member] = (x, y)   # (after the call: a refused submit leaves sofa_output(member) the array the outstanding ticket fills)
        else:
            self._ck(self.L.mi355_agroup_submit_sofa(self.h, member, inp, out, n_blocks, g.ctypes.data_as(fp), 1, C.byref(t)))
        return t.value

    def sofa_output(self, member):
        """the output array of the member's last host submission (filled by wait)"""
        return self._keep[member][1]

    def sofa_info(self, member):
        """(filter partitions K, transform size 2 * partition_length, filters pending)"""
        k, n, pend = C.c_int(0), C.c_int(0), C.c_int(0)
        self._ck(self.L.mi355_agroup_sofa_info(self.h, member, C.byref(k), C.byref(n), C.byref(pend)))
        return k.value, n.value, pend.value

    def sofa_launches(self):
        return int(self.L.mi355_agroup_sofa_launches(self.h))

    # ---- mixer members (minus1mixer / audiomultimixer)
    def mixer_setup(self, member, contrib):
        """contrib: bool matrix [n_inputs, n_out_channels] of one member"""
        m = np.ascontiguousarray(np.asarray(contrib) != 0, dtype=np.uint8)
        self._ck(self.L.mi355_agroup_mixer_setup(self.h, member, m.shape[0], m.shape[1], m.ctypes.data))

    def mixer_setup_minus1(self, member, n_streams):
        self._ck(self.L.mi355_agroup_mixer_setup_minus1(self.h, member, n_streams))

    def submit_mixer(self, member, segments, outputs, frames, device_data=False):
        """One interval of one member; segments / outputs as mixer_tables takes them. Host outputs are filled by wait."""
        segs, outs = mixer_tables(segments, outputs)
        t = C.c_uint64(0)
        self._ck(self.L.mi355_agroup_submit_mixer(self.h, member, segs, len(segments), outs, len(outputs), frames, int(bool(device_data)), C.byref(t)))
        self._keep[member] = (segments, outputs)   # (after the call: a refused submit leaves the buffers of the outstanding ticket alone)
        return t.value

    def mixer_launches(self):
        return int(self.L.mi355_agroup_mixer_launches(self.h))

    def submit_ebur128(self, member, data, frames=None, sample_format=None):
        t = C.c_uint64(0)
        if isinstance(data, np.ndarray):
            fmt = {np.dtype(np.int16): 0, np.dtype(np.int32): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}[data.dtype]
            assert data.flags.c_contiguous
            self._ck(self.L.mi355_agroup_submit_ebur128(self.h, member, data.ctypes.data, data.size // self.channels, fmt, 0, C.byref(t)))
            self._keep[member] = data
        else:
            self._ck(self.L.mi355_agroup_submit_ebur128(self.h, member, data, frames, sample_format, 1, C.byref(t)))
        return t.value

    def ebur128_reset(self, member):
        """the `reset` action of one ebur128level instance: this member's meter starts over, the others are not touched"""
        self._ck(self.L.mi355_agroup_ebur128_reset(self.h, member))

    def loudnorm_frame_size(self, member=0):
        """the frame `member` hands over next: its first 3 s, then 100 ms"""
        return int(self.L.mi355_agroup_loudnorm_frame_size(self.h, member))

    def submit_loudnorm(self, member, data, out, final_frame=False, frames=None, out_capacity_frames=None):
        """data / out: numpy f64 arrays [frames, channels] (host) or device pointers (then frames, out_capacity_frames)."""
        t = C.c_uint64(0)
        if isinstance(out, np.ndarray):
            data = np.ascontiguousarray(data, dtype=np.float64)
            assert out.flags.c_contiguous and out.dtype == np.float64
            self._ck(self.L.mi355_agroup_submit_loudnorm(self.h, member, data.ctypes.data if data.size else None, data.size // self.channels, out.ctypes.data,
                                                         out.size // self.channels, int(bool(final_frame)), 0, C.byref(t)))
            self._keep[member] = (data, out)
        else:
            self._ck(self.L.mi355_agroup_submit_loudnorm(self.h, member, data, frames, out, out_capacity_frames, int(bool(final_frame)), 1, C.byref(t)))
        return t.value

    def wait(self, ticket):
        n = C.c_size_t(0)
        self._ck(self.L.mi355_agroup_wait(self.h, ticket, C.byref(n)))
        return int(n.value)

    def loudness(self, member, what):
        d = C.c_double(0.0)
        self._ck(self.L.mi355_agroup_ebur128_loudness(self.h, member, what, C.byref(d)))
        return d.value

    def peak(self, member, channel, true_peak=False):
        d = C.c_double(0.0)
        self._ck(self.L.mi355_agroup_ebur128_peak(self.h, member, int(bool(true_peak)), channel, C.byref(d)))
        return d.value

    def echo_state(self, member, ring_len):
        ring = np.zeros(ring_len, dtype=np.float64)
        pos = C.c_size_t(0)
        self._ck(self.L.mi355_agroup_echo_get_state(self.h, member, ring.ctypes.data, ring_len, C.byref(pos)))
        return ring, int(pos.value)

    def stats(self):
        c = (C.c_uint64 * 3)()
        self._ck(self.L.mi355_agroup_stats(self.h, c))
        return int(c[0]), int(c[1]), int(c[2])

    def loudnorm_push(self, member, data):
        """mi355_agroup_loudnorm_push: the member's sink_chain (adapter on the library's side). -> output samples of the frames completed."""
        a = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
        frames = a.size // self.channels
        cap = (frames // 19200 + 32) * 19200
        out = np.zeros(cap * self.channels, np.float64)
        n = C.c_size_t(0)
        self._ck(self.L.mi355_agroup_loudnorm_push(self.h, member, a.ctypes.data, frames, out.ctypes.data, cap, C.byref(n)))
        return out[: n.value * self.channels]

    def loudnorm_drain(self, member):
        cap = 31 * 19200 + 3 * 192000
        out = np.zeros(cap * self.channels, np.float64)
        n, eos = C.c_size_t(0), C.c_int(0)
        self._ck(self.L.mi355_agroup_loudnorm_drain(self.h, member, out.ctypes.data, cap, C.byref(n), C.byref(eos)))
        return None if eos.value else out[: n.value * self.channels]

    def close(self):
        if self.h:
            if self.shared:
                self.L.mi355_agroup_release(self.h, self.member)
            else:
                self.L.mi355_agroup_destroy(self.h)
            self.h = None


class Context:
    """One element instance's device context (mi355_ctx)."""

    def __init__(self, device=0):
        self.L = load_library()
        st = C.c_int(0)
        self.h = self.L.mi355_ctx_create(device, C.byref(st))
        if not self.h:
            raise Mi355Error(st.value, self.L.mi355_status_string(st.value).decode())
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.L.mi355_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        if rc != 0:
            raise Mi355Error(rc, self.L.mi355_ctx_last_error(self.h).decode("utf-8", "replace"))

    # ---- plumbing
    @property
    def stream(self):
        return self.L.mi355_ctx_stream(self.h)

    def set_stream(self, hip_stream):
        self._ck(self.L.mi355_ctx_set_stream(self.h, hip_stream))

    def synchronize(self):
        self._ck(self.L.mi355_ctx_synchronize(self.h))

    def set_flag(self, flag, value):
        self._ck(self.L.mi355_ctx_set_flag(self.h, flag, int(value)))

    def alloc(self, nbytes):
        p = self.L.mi355_device_alloc(self.h, nbytes)
        if not p:
            raise Mi355Error(ERR_OOM, self.L.mi355_ctx_last_error(self.h).decode())
        return p

    def free(self, dptr):
        self._ck(self.L.mi355_device_free(self.h, dptr))

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._ck(self.L.mi355_memcpy_h2d(self.h, dptr, arr.ctypes.data, arr.nbytes))

    def d2h(self, arr, dptr):
        assert arr.flags.c_contiguous
        self._ck(self.L.mi355_memcpy_d2h(self.h, arr.ctypes.data, dptr, arr.nbytes))

    def chain_batches_device(self, src_ptrs, dst_ptrs, n_frames, frame_pitch, stride, width, height, fmt, settings, lanes=1):
        """hsvfilter in place + colorlut for len(src_ptrs) independent batches from one native call (lanes: 1 or 2 streams)."""
        key = (tuple(src_ptrs), tuple(dst_ptrs))
        arr = self._chain_arrays.get(key) if hasattr(self, "_chain_arrays") else None
        if arr is None:
            if not hasattr(self, "_chain_arrays"):
                self._chain_arrays = {}
            n = len(src_ptrs)
            arr = self._chain_arrays[key] = ((C.c_void_p * n)(*src_ptrs), (C.c_void_p * n)(*dst_ptrs))
        hs = HsvSettings(*[float(v) for v in settings])
        self._ck(self.L.mi355_hsv_colorlut_chain_batches_device(self.h, arr[0], arr[1], len(src_ptrs), n_frames, frame_pitch, stride, width, height,
                                                                FMT[fmt], C.byref(hs), lanes))

    # ---- device buffers (what a device GstMemory wraps) and transfer accounting
    def buf_alloc(self, nbytes):
        b = self.L.mi355_buf_alloc(self.h, nbytes)
        if not b:
            raise Mi355Error(ERR_OOM, self.L.mi355_ctx_last_error(self.h).decode())
        return DeviceBuffer(self, b)

    def transfer_counts(self):
        """(host->device, device->host) copies this context's buffers and copy entry points have enqueued so far."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.mi355_ctx_transfer_counts(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    # ---- roundedcorners: the host-rendered alpha plane kept in HBM
    def roundedcorners_set_mask(self, mask, width, height, stride):
        if mask is None:
            self._ck(self.L.mi355_roundedcorners_set_mask(self.h, None, 0, 0, 0))
        else:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            assert mask.size >= stride * ((height + 1) & ~1)
            self._ck(self.L.mi355_roundedcorners_set_mask(self.h, mask.ctypes.data, width, height, stride))

    def roundedcorners_mask_device(self):
        p, n, st = C.c_void_p(), C.c_size_t(0), C.c_int(0)
        self._ck(self.L.mi355_roundedcorners_mask_device(self.h, C.byref(p), C.byref(n), C.byref(st)))
        return p.value, int(n.value), int(st.value)

    def roundedcorners_append_device(self, d_frames, frame_pitch, alpha_offset, n_frames):
        self._ck(self.L.mi355_roundedcorners_append_device(self.h, d_frames, frame_pitch, alpha_offset, n_frames))

    # ---- hsvfilter
    def hsvfilter_frame_ip(self, data, width, stride, fmt, settings, data_len=None):
        s = HsvSettings(*[float(v) for v in settings])
        n = data.nbytes if data_len is None else data_len
        self._ck(self.L.mi355_hsvfilter_frame_ip(self.h, _ptr(data), n, width, stride, FMT[fmt], C.byref(s)))
        return data

    def hsvfilter_frames_device(self, dptr, n_frames, frame_pitch, width, height, stride, fmt, settings):
        s = HsvSettings(*[float(v) for v in settings])
        self._ck(self.L.mi355_hsvfilter_frames_device(self.h, dptr, n_frames, frame_pitch, width, height, stride, FMT[fmt], C.byref(s)))

    def time_hsvfilter_device(self, dptr, n_frames, frame_pitch, width, height, stride, fmt, settings, iters):
        s = HsvSettings(*[float(v) for v in settings])
        ms = C.c_float(0)
        self._ck(self.L.mi355_time_hsvfilter_device(self.h, dptr, n_frames, frame_pitch, width, height, stride, FMT[fmt], C.byref(s), iters, C.byref(ms)))
        return ms.value

    # ---- hsvdetector
    def hsvdetect_frame(self, src, src_stride, src_fmt, dst, dst_stride, dst_fmt, width, settings):
        s = HsvDetectSettings(*[float(v) for v in settings])
        self._ck(self.L.mi355_hsvdetect_frame(self.h, _ptr(src), src.nbytes, src_stride, FMT[src_fmt], _ptr(dst), dst.nbytes,
                                              dst_stride, FMT[dst_fmt], width, C.byref(s)))
        return dst

    def hsvdetect_frames_device(self, d_src, src_pitch, src_stride, src_fmt, d_dst, dst_pitch, dst_stride, dst_fmt, n_frames, width, height, settings):
        """n_frames device frames on this context's stream (asynchronous: synchronize() before reading d_dst back)."""
        s = None if settings is None else C.byref(HsvDetectSettings(*[float(v) for v in settings]))
        self._ck(self.L.mi355_hsvdetect_frames_device(self.h, d_src, src_pitch, src_stride, FMT[src_fmt], d_dst, dst_pitch, dst_stride, FMT[dst_fmt],
                                                      n_frames, width, height, s))

    # ---- colorlut
    def colorlut_load(self, is3d, size, table, scale=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0)):
        t = np.ascontiguousarray(table, dtype=np.float32).ravel()
        assert t.size == (4 * size ** 3 if is3d else 3 * size), "table size mismatch"
        sc = np.ascontiguousarray(scale, dtype=np.float32)
        of = np.ascontiguousarray(offset, dtype=np.float32)
        fp = C.POINTER(C.c_float)
        self._ck(self.L.mi355_colorlut_load(self.h, int(is3d), size, t.ctypes.data_as(fp), sc.ctypes.data_as(fp), of.ctypes.data_as(fp)))

    def colorlut_unload(self):
        self._ck(self.L.mi355_colorlut_unload(self.h))

    def colorlut_kernel_choice(self, fused=False):
        """(table_in_use, ms per megapixel of the interpolating kernel, of the table kernel) for LUT variant 0 (auto)."""
        k, a, b = C.c_int(0), C.c_double(0), C.c_double(0)
        self._ck(self.L.mi355_colorlut_kernel_choice(self.h, int(fused), C.byref(k), C.byref(a), C.byref(b)))
        return bool(k.value), a.value, b.value

    def colorlut_kernel_name(self):
        """Name of the kernel that served the last colorlut / fused launch of this context."""
        return (self.L.mi355_colorlut_last_kernel(self.h) or b"").decode()

    def colorlut_brick_stats(self, reset=False):
        """(steps with a miss, steps on the slow path, last miss fraction seen by the content watch, level it settled on)."""
        c = (C.c_uint64 * 2)()
        f, h = C.c_double(0), C.c_int(0)
        self._ck(self.L.mi355_colorlut_brick_stats(self.h, c, C.byref(f), C.byref(h), int(reset)))
        return int(c[0]), int(c[1]), f.value, int(h.value)

    def colorlut_window_stats(self, reset=False):
        """LDS-cached table kernel: (pixels looked up, pixels served past the LDS cache, bricks installed) since the last reset."""
        c = (C.c_uint64 * 3)()
        self._ck(self.L.mi355_colorlut_window_stats(self.h, c, int(reset)))
        return int(c[0]), int(c[1]), int(c[2])

    def colorlut_frame(self, src, src_stride, dst, dst_stride, width, height, fmt="RGBA"):
        self._ck(self.L.mi355_colorlut_frame(self.h, _ptr(src), src_stride, _ptr(dst), dst_stride, width, height, FMT[fmt]))
        return dst

    def colorlut_frames_device(self, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, n_frames, width, height, fmt="RGBA"):
        self._ck(self.L.mi355_colorlut_frames_device(self.h, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, n_frames, width, height, FMT[fmt]))

    def time_colorlut_device(self, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, n_frames, width, height, fmt, iters):
        ms = C.c_float(0)
        self._ck(self.L.mi355_time_colorlut_device(self.h, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, n_frames, width, height, FMT[fmt], iters, C.byref(ms)))
        return ms.value

    # ---- hsvfilter ! colorlut as one pass (RGBA)
    def hsv_colorlut_frames_device(self, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, n_frames, width, height, settings):
        s = HsvSettings(*[float(v) for v in settings])
        self._ck(self.L.mi355_hsv_colorlut_frames_device(self.h, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, n_frames, width, height, C.byref(s)))

    def time_hsv_colorlut_device(self, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, n_frames, width, height, settings, iters):
        s = HsvSettings(*[float(v) for v in settings])
        ms = C.c_float(0)
        self._ck(self.L.mi355_time_hsv_colorlut_device(self.h, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, n_frames, width, height, C.byref(s), iters, C.byref(ms)))
        return ms.value

    # ---- audioloudnorm (interleaved f64 @ 192 kHz)
    def loudnorm_setup(self, channels, loudness_target=-24.0, loudness_range_target=7.0, max_true_peak=-2.0, offset=0.0):
        self._ck(self.L.mi355_loudnorm_setup(self.h, channels, loudness_target, loudness_range_target, max_true_peak, offset))
        self._ln_channels = channels

    def loudnorm_push(self, data):
        a = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
        frames = a.size // self._ln_channels
        cap = (frames // 19200 + 32) * 19200
        out = np.zeros(cap * self._ln_channels, np.float64)
        n = C.c_size_t(0)
        self._ck(self.L.mi355_loudnorm_push(self.h, a.ctypes.data, frames, out.ctypes.data, cap, C.byref(n)))
        return out[: n.value * self._ln_channels]

    def loudnorm_drain(self):
        cap = 31 * 19200 + 3 * 192000
        out = np.zeros(cap * self._ln_channels, np.float64)
        n, eos = C.c_size_t(0), C.c_int(0)
        self._ck(self.L.mi355_loudnorm_drain(self.h, out.ctypes.data, cap, C.byref(n), C.byref(eos)))
        return None if eos.value else out[: n.value * self._ln_channels]

    def loudnorm_teardown(self):
        self._ck(self.L.mi355_loudnorm_teardown(self.h))

    # ---- audioloudnorm, n streams in lock step
    def loudnorm_setup_batch(self, n_streams, channels, loudness_target=-24.0, loudness_range_target=7.0, max_true_peak=-2.0, offset=0.0):
        self._ck(self.L.mi355_loudnorm_setup_batch(self.h, n_streams, channels, loudness_target, loudness_range_target, max_true_peak, offset))
        self._lnb = (n_streams, channels)

    def loudnorm_batch_frame_size(self):
        return int(self.L.mi355_loudnorm_batch_frame_size(self.h))

    def loudnorm_process_batch(self, data, final=False):
        """data: (n_streams, frames * channels) float64, one frame (or, final, the shorter rest) per stream. -> (n_streams, out_frames * channels)."""
        S, ch = self._lnb
        a = np.ascontiguousarray(data, dtype=np.float64).reshape(S, -1)
        frames = a.shape[1] // ch
        cap = 31 * 19200 if final else max(frames, 19200)
        out = np.zeros((S, cap * ch), np.float64)
        n = C.c_size_t(0)
        self._ck(self.L.mi355_loudnorm_process_batch(self.h, a.ctypes.data if a.size else None, a.shape[1], frames, out.ctypes.data, cap * ch, cap, C.byref(n), int(final), 0))
        return out[:, : n.value * ch]

    def loudnorm_process_batch_device(self, d_in, stream_stride, frames, d_out, out_stride, cap_frames, final=False):
        n = C.c_size_t(0)
        self._ck(self.L.mi355_loudnorm_process_batch(self.h, d_in, stream_stride, frames, d_out, out_stride, cap_frames, C.byref(n), int(final), 1))
        return n.value

    # ---- pinned host memory + asynchronous host-buffer pipeline
    def host_array(self, nbytes):
        """A page-locked uint8 numpy array of `nbytes` (mi355_host_alloc); free with host_free(arr)."""
        p = self.L.mi355_host_alloc(self.h, nbytes)
        if not p:
            raise Mi355Error(ERR_OOM, self.L.mi355_ctx_last_error(self.h).decode("utf-8", "replace"))
        arr = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        p = self._pinned.pop(arr.ctypes.data)
        self._ck(self.L.mi355_host_free(self.h, p))

    def pipe_create(self, depth, max_frame_bytes):
        p = self.L.mi355_pipe_create(self.h, depth, max_frame_bytes)
        if not p:
            raise Mi355Error(ERR_INVALID_ARG, self.L.mi355_ctx_last_error(self.h).decode("utf-8", "replace"))
        return p

    def pipe_destroy(self, pipe):
        self.L.mi355_pipe_destroy(pipe)

    def pipe_submit_hsvfilter(self, pipe, data, width, stride, fmt, settings):
        s = HsvSettings(*[float(v) for v in settings])
        t = C.c_uint64(0)
        self._ck(self.L.mi355_pipe_submit_hsvfilter(pipe, _ptr(data), data.nbytes, width, stride, FMT[fmt], C.byref(s), C.byref(t)))
        return t.value

    def pipe_submit_colorlut(self, pipe, src, src_stride, dst, dst_stride, width, height, fmt="RGBA"):
        t = C.c_uint64(0)
        self._ck(self.L.mi355_pipe_submit_colorlut(pipe, _ptr(src), src_stride, _ptr(dst), dst_stride, width, height, FMT[fmt], C.byref(t)))
        return t.value

    def pipe_submit_hsv_colorlut(self, pipe, src, src_stride, dst, dst_stride, width, height, settings):
        s = HsvSettings(*[float(v) for v in settings])
        t = C.c_uint64(0)
        self._ck(self.L.mi355_pipe_submit_hsv_colorlut(pipe, _ptr(src), src_stride, _ptr(dst), dst_stride, width, height, C.byref(s), C.byref(t)))
        return t.value

    def pipe_set_group(self, pipe, group):
        """The pipe's hsv+colorlut frames go through `group` (a Group, or None for the pipe's own launches)."""
        self._ck(self.L.mi355_pipe_set_group(pipe, group.h if group is not None else None))

    def pipe_wait(self, pipe, ticket):
        self._ck(self.L.mi355_pipe_wait(pipe, ticket))

    def pipe_wait_all(self, pipe):
        self._ck(self.L.mi355_pipe_wait_all(pipe))

    # ---- colordetect: color_thief::get_palette of plane 0 (video/videofx/src/colordetect/imp.rs:57-84)
    COLORDETECT_FORMATS = ("RGB", "RGBA", "ARGB", "BGR", "BGRA")

    def colordetect_frame(self, data, fmt, quality=10, max_colors=2):
        """[(r, g, b), ...] in palette order for a host plane (any contiguous uint8 array, read as a flat byte run)."""
        a = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        pal = np.zeros(255 * 3, np.uint8)
        n = C.c_int(0)
        self._ck(self.L.mi355_colordetect_frame(self.h, a.ctypes.data, a.nbytes, FMT[fmt], quality, max_colors, pal.ctypes.data, C.byref(n)))
        return [tuple(int(x) for x in pal[3 * k:3 * k + 3]) for k in range(n.value)]

    def colordetect_frames_device(self, d_frames, frame_pitch, data_len, n_frames, fmt, quality=10, max_colors=2):
        """One palette per device plane d_frames + f * frame_pitch; one synchronisation."""
        pal = np.zeros(max(n_frames, 1) * 255 * 3, np.uint8)
        n = (C.c_int * max(n_frames, 1))()
        self._ck(self.L.mi355_colordetect_frames_device(self.h, d_frames, frame_pitch, data_len, n_frames, FMT[fmt], quality, max_colors,
                                                        pal.ctypes.data, n))
        return [[tuple(int(x) for x in pal[(f * 255 + k) * 3:(f * 255 + k) * 3 + 3]) for k in range(n[f])] for f in range(n_frames)]

    def colordetect_histogram_device(self, d_data, data_len, fmt, quality=10):
        """(32768 bins as uint32, first box (r1, r2, g1, g2, b1, b2) or None when no sample is kept)."""
        hist = np.zeros(32768, np.uint32)
        box = (C.c_int * 6)()
        self._ck(self.L.mi355_colordetect_histogram_device(self.h, d_data, data_len, FMT[fmt], quality,
                                                           hist.ctypes.data_as(C.POINTER(C.c_uint32)), box))
        b = tuple(box[k] for k in range(6))
        return hist, (None if b[0] < 0 else b)

    def selftest_colordetect_mmcq(self, bins, max_colors):
        """Test only: (palette, first box or None) of the MMCQ kernel run on 32768 bins given by the caller."""
        h = np.ascontiguousarray(bins, dtype=np.uint32).reshape(-1)
        assert h.size == 32768
        pal = np.zeros(255 * 3, np.uint8)
        n = C.c_int(0)
        box = (C.c_int * 6)()
        self._ck(self.L.mi355_selftest_colordetect_mmcq(self.h, h.ctypes.data, max_colors, pal.ctypes.data, C.byref(n), box))
        b = tuple(box[k] for k in range(6))
        return [tuple(int(x) for x in pal[3 * k:3 * k + 3]) for k in range(n.value)], (None if b[0] < 0 else b)

    # ---- videocompare
    HASH_ALGO = {"mean": 0, "gradient": 1, "vertgradient": 2, "doublegradient": 3, "blockhash": 4, "dssim": 5}

    def videocompare_hash_frame(self, frame, stride, width, height, fmt="RGBA", algo="blockhash"):
        h = C.c_uint64(0)
        self._ck(self.L.mi355_videocompare_hash_frame(self.h, _ptr(frame), stride, width, height, FMT[fmt], self.HASH_ALGO[algo], C.byref(h)))
        return h.value

    def videocompare_hash_frames_device(self, d_frames, frame_pitch, stride, n_frames, width, height, fmt="RGBA", algo="blockhash"):
        hs = (C.c_uint64 * max(n_frames, 1))()
        self._ck(self.L.mi355_videocompare_hash_frames_device(self.h, d_frames, frame_pitch, stride, n_frames, width, height, FMT[fmt],
                                                              self.HASH_ALGO[algo], hs))
        return [hs[k] for k in range(n_frames)]

    def videocompare_distance(self, a, b, algo="blockhash"):
        return self.L.mi355_videocompare_distance(self.HASH_ALGO[algo], a, b)

    # ---- videocompare: Dssim engine
    def dssim_create_image(self, frame, stride, width, height, fmt="RGBA"):
        h = C.c_void_p()
        self._ck(self.L.mi355_dssim_create_image(self.h, _ptr(frame), stride, width, height, FMT[fmt], C.byref(h)))
        return h

    def dssim_create_image_device(self, d_frame, stride, width, height, fmt="RGBA"):
        h = C.c_void_p()
        self._ck(self.L.mi355_dssim_create_image_device(self.h, d_frame, stride, width, height, FMT[fmt], C.byref(h)))
        return h

    def dssim_free_image(self, img):
        self.L.mi355_dssim_free_image(self.h, img)

    def dssim_image_plane(self, img, scale, channel, kind):
        """kind: 'img' | 'mu' | 'sq' -> (h, w) float32 array copied from the device image."""
        w, h = C.c_int(0), C.c_int(0)
        k = {"img": 0, "mu": 1, "sq": 2}[kind]
        self._ck(self.L.mi355_dssim_image_plane(self.h, img, scale, channel, k, None, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.float32)
        self._ck(self.L.mi355_dssim_image_plane(self.h, img, scale, channel, k, out.ctypes.data_as(C.POINTER(C.c_float)), None, None))
        return out

    def dssim_compare_frames(self, original, frames, stride, width, height, fmt="RGBA"):
        """videocompare's loop over the non-reference pads: hash + compare each host frame against `original` in one pass."""
        n = len(frames)
        ptrs = (C.c_void_p * max(n, 1))(*[f.ctypes.data for f in frames])
        out = (C.c_double * max(n, 1))()
        self._ck(self.L.mi355_dssim_compare_frames(self.h, original, ptrs, n, stride, width, height, FMT[fmt], out))
        return [out[k] for k in range(n)]

    def dssim_compare_frames_device(self, original, d_frames, stride, width, height, fmt="RGBA"):
        n = len(d_frames)
        ptrs = (C.c_void_p * max(n, 1))(*[int(d) for d in d_frames])
        out = (C.c_double * max(n, 1))()
        self._ck(self.L.mi355_dssim_compare_frames_device(self.h, original, ptrs, n, stride, width, height, FMT[fmt], out))
        return [out[k] for k in range(n)]

    def dssim_compare_pairs(self, refs, frames, stride, width, height, fmt="RGBA"):
        """n independent (reference, frame) pairs of host frames -> their dssim values; exact or fast by FLAG_DSSIM_FAST."""
        n = len(frames)
        if len(refs) != n:
            raise ValueError("dssim_compare_pairs: as many references as frames")
        pr = (C.c_void_p * max(n, 1))(*[f.ctypes.data for f in refs])
        pf = (C.c_void_p * max(n, 1))(*[f.ctypes.data for f in frames])
        out = (C.c_double * max(n, 1))()
        self._ck(self.L.mi355_dssim_compare_pairs(self.h, pr, pf, n, stride, width, height, FMT[fmt], out))
        return [out[k] for k in range(n)]

    def dssim_compare_pairs_device(self, d_refs, d_frames, stride, width, height, fmt="RGBA"):
        n = len(d_frames)
        if len(d_refs) != n:
            raise ValueError("dssim_compare_pairs_device: as many references as frames")
        pr = (C.c_void_p * max(n, 1))(*[int(d) for d in d_refs])
        pf = (C.c_void_p * max(n, 1))(*[int(d) for d in d_frames])
        out = (C.c_double * max(n, 1))()
        self._ck(self.L.mi355_dssim_compare_pairs_device(self.h, pr, pf, n, stride, width, height, FMT[fmt], out))
        return [out[k] for k in range(n)]

    def dssim_pair_map_device(self, d_ref, d_frame, stride, width, height, fmt="RGBA", scale=0, out=None):
        """(h, w) float32 SSIM map of one scale of one pair of device frames, in the form FLAG_DSSIM_FAST selects. `out`: a
        C-contiguous float32 array with at least h * w elements to receive it (the first h * w are written)."""
        w, h = C.c_int(0), C.c_int(0)
        self._ck(self.L.mi355_dssim_pair_map_device(self.h, int(d_ref), int(d_frame), stride, width, height, FMT[fmt], scale, None, C.byref(w), C.byref(h)))
        if out is None:
            out = np.zeros((h.value, w.value), np.float32)
        elif out.dtype != np.float32 or not out.flags.c_contiguous or out.size < h.value * w.value:
            raise ValueError("dssim_pair_map_device: out must be C-contiguous float32 of at least %d elements" % (h.value * w.value))
        self._ck(self.L.mi355_dssim_pair_map_device(self.h, int(d_ref), int(d_frame), stride, width, height, FMT[fmt], scale, out.ctypes.data_as(C.POINTER(C.c_float)), None, None))
        return out

    def selftest_dssim_cbrt(self, lo, hi):
        """Mismatches between the kernels' cube root and the literal one over every f32 in [lo, hi] (both > 0)."""
        n = C.c_uint64(0)
        lo_bits, hi_bits = (int(np.float32(v).view(np.uint32)) for v in (lo, hi))
        self._ck(self.L.mi355_selftest_dssim_cbrt(self.h, lo_bits, hi_bits, C.byref(n)))
        return n.value

    def dssim_compare(self, a, b):
        v = C.c_double(0)
        self._ck(self.L.mi355_dssim_compare(self.h, a, b, C.byref(v)))
        return v.value

    def selftest_dssim_compare_detail(self, a, b, scale):
        """dssim_compare(a, b) with the insides of one scale: (value, (h, w) float32 SSIM map, [sum, avg, dev])."""
        w, h = C.c_int(0), C.c_int(0)
        self._ck(self.L.mi355_dssim_image_plane(self.h, a, scale, 0, 0, None, C.byref(w), C.byref(h)))
        m = np.full((h.value, w.value), np.nan, np.float32)
        slots, v = (C.c_double * 3)(), C.c_double(0)
        self._ck(self.L.mi355_selftest_dssim_compare_detail(self.h, a, b, scale, m.ctypes.data_as(C.POINTER(C.c_float)), slots, C.byref(v)))
        return v.value, m, list(slots)

    # ---- sofalizer
    def sofa_setup(self, channels, filter_len, partition_length=64, block_length=256):
        self._ck(self.L.mi355_sofa_setup(self.h, channels, filter_len, partition_length, block_length))
        self._sofa = (channels, block_length)

    def sofa_set_filter(self, channel, left, right, delay_left=0, delay_right=0):
        fp = C.POINTER(C.c_float)
        l, r = np.ascontiguousarray(left, np.float32), np.ascontiguousarray(right, np.float32)
        self._ck(self.L.mi355_sofa_set_filter(self.h, channel, l.ctypes.data_as(fp), r.ctypes.data_as(fp), delay_left, delay_right))

    def sofa_set_drop(self, channel, drop=True):
        self._ck(self.L.mi355_sofa_set_drop(self.h, channel, int(drop)))

    def sofa_reset(self):
        self._ck(self.L.mi355_sofa_reset(self.h))

    def sofa_teardown(self):
        self._ck(self.L.mi355_sofa_teardown(self.h))

    def sofa_process_block(self, block, gains):
        """block: (block_length, channels) f32 -> (block_length, 2) f32."""
        fp = C.POINTER(C.c_float)
        ch, bl = self._sofa
        x = np.ascontiguousarray(block, np.float32).reshape(bl, ch)
        g = np.ascontiguousarray(gains, np.float32)
        out = np.zeros((bl, 2), np.float32)
        self._ck(self.L.mi355_sofa_process_block(self.h, x.ctypes.data_as(fp), out.ctypes.data_as(fp), g.ctypes.data_as(fp)))
        return out

    def sofa_process_block_device(self, d_in, d_out, gains):
        fp = C.POINTER(C.c_float)
        g = np.ascontiguousarray(gains, np.float32)
        self._ck(self.L.mi355_sofa_process_block_device(self.h, d_in, d_out, g.ctypes.data_as(fp)))

    # ---- hrtfrender
    def hrtf_load_sphere(self, data, rate):
        b = bytes(data)
        buf = (C.c_uint8 * len(b)).from_buffer_copy(b)
        self._ck(self.L.mi355_hrtf_load_sphere(self.h, C.cast(buf, C.c_void_p), len(b), rate))

    def hrtf_setup(self, channels, block_length=512, interpolation_steps=8):
        self._ck(self.L.mi355_hrtf_setup(self.h, channels, block_length, interpolation_steps))
        self._hrtf_shape = (channels, block_length * interpolation_steps, interpolation_steps)

    def hrtf_reset(self):
        self._ck(self.L.mi355_hrtf_reset(self.h))

    def hrtf_teardown(self):
        self._ck(self.L.mi355_hrtf_teardown(self.h))

    def hrtf_sphere_info(self):
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._ck(self.L.mi355_hrtf_sphere_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def hrtf_transform_size(self):
        """overlap-save transform size setup chose, 0 when the time-domain FIR serves"""
        n = C.c_int(-1)
        self._ck(self.L.mi355_hrtf_transform_size(self.h, C.byref(n)))
        return n.value

    def hrtf_process_block(self, inp, positions, gains):
        channels, frames, _ = self._hrtf_shape
        fp = C.POINTER(C.c_float)
        x = np.ascontiguousarray(inp, dtype=np.float32).reshape(-1)
        assert x.size == frames * channels, "one block = block_length*interpolation_steps frames"
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1)
        g = np.ascontiguousarray(gains, dtype=np.float32).reshape(-1)
        assert pos.size == 3 * channels and g.size == channels
        out = np.zeros(frames * 2, np.float32)
        self._ck(self.L.mi355_hrtf_process_block(self.h, x.ctypes.data_as(fp), out.ctypes.data_as(fp), pos.ctypes.data_as(fp), g.ctypes.data_as(fp)))
        return out

    def hrtf_process_block_device(self, d_in, d_out, positions, gains):
        fp = C.POINTER(C.c_float)
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1)
        g = np.ascontiguousarray(gains, dtype=np.float32).reshape(-1)
        self._ck(self.L.mi355_hrtf_process_block_device(self.h, d_in, d_out, pos.ctypes.data_as(fp), g.ctypes.data_as(fp)))

    def hrtf_last_lookup(self):
        channels, _, steps = self._hrtf_shape
        faces = np.zeros(channels * steps, np.int32)
        uvw = np.zeros(channels * steps * 3, np.float32)
        self._ck(self.L.mi355_hrtf_last_lookup(self.h, faces.ctypes.data_as(C.POINTER(C.c_int)), uvw.ctypes.data_as(C.POINTER(C.c_float))))
        return faces.reshape(channels, steps), uvw.reshape(channels, steps, 3)

    # ---- agingradio
    def agingradio_setup(self, channels, rate, lowpass_freq, seed):
        self._ck(self.L.mi355_agingradio_setup(self.h, channels, rate, lowpass_freq, seed))

    def agingradio_reset(self):
        self._ck(self.L.mi355_agingradio_reset(self.h))

    def agingradio_process(self, data, channels, settings):
        """in place on a numpy f32 / f64 array of frames * channels interleaved samples; settings: dict (defaults for missing keys)"""
        assert data.dtype in (np.float32, np.float64) and data.flags.c_contiguous
        st = AgingRadioSettings.of(settings)
        self._ck(self.L.mi355_agingradio_process(self.h, data.ctypes.data, data.size // channels, int(data.dtype == np.float64), C.byref(st)))
        return data

    def agingradio_process_device(self, dptr, frames, is_f64, settings):
        st = AgingRadioSettings.of(settings)
        self._ck(self.L.mi355_agingradio_process_device(self.h, dptr, frames, int(bool(is_f64)), C.byref(st)))

    def agingradio_state(self, channels):
        """(the filters' outputs, frame pairs processed since setup)"""
        y = np.zeros(max(channels, 1), np.float64)
        k = C.c_uint64(0)
        self._ck(self.L.mi355_agingradio_get_state(self.h, y.ctypes.data_as(C.POINTER(C.c_double)), channels, C.byref(k)))
        return y[:channels], int(k.value)

    # ---- minus1mixer / audiomultimixer
    def mixer_setup(self, contrib):
        """contrib: bool matrix [n_inputs, n_out_channels]"""
        m = np.ascontiguousarray(np.asarray(contrib) != 0, dtype=np.uint8)
        self._ck(self.L.mi355_mixer_setup(self.h, m.shape[0], m.shape[1], m.ctypes.data))

    def mixer_setup_minus1(self, n_streams):
        self._ck(self.L.mi355_mixer_setup_minus1(self.h, n_streams))

    def mixer_reset(self):
        self._ck(self.L.mi355_mixer_reset(self.h))

    def mixer_process(self, segments, outputs, frames):
        """One interval on host memory: segments / outputs as mixer_tables takes them (numpy arrays); the output arrays are filled."""
        segs, outs = mixer_tables(segments, outputs)
        self._ck(self.L.mi355_mixer_process(self.h, segs, len(segments), outs, len(outputs), frames))

    def mixer_process_device(self, segments, outputs, frames):
        """The same on device memory (pointer forms of mixer_tables), enqueued on the context's stream."""
        segs, outs = mixer_tables(segments, outputs)
        self._ck(self.L.mi355_mixer_process_device(self.h, segs, len(segments), outs, len(outputs), frames))

    # ---- yolov8tensordec2 / yoloxtensordec (analytics/analytics/src/yolotensordec/imp.rs:234-422)
    def yolodec(self, tensor, layout, params, max_dets=None, return_count=False):
        """The kept boxes of one host tensor as a YOLO_DET record array, in output order. tensor: float32, (F, N) for layout "V8",
        (N, F) for "X" (a leading batch axis of 1 is accepted); params: (box_thr, class_thr, iou_thr). max_dets: the capacity of
        the result (default N: never truncated); with return_count the full kept count comes back as well."""
        a = np.ascontiguousarray(tensor, dtype=np.float32)
        if a.ndim == 3 and a.shape[0] == 1:
            a = a[0]
        if a.ndim != 2:
            raise ValueError("yolodec: a [F, N] (V8) or [N, F] (X) tensor")
        F, N = (a.shape if layout == "V8" else a.shape[::-1])
        cap = N if max_dets is None else max_dets
        p, _ = _yolo_params(params)
        dets = np.zeros(max(cap, 1), YOLO_DET)
        n = C.c_uint32(0)
        self._ck(self.L.mi355_yolodec_tensor(self.h, a.ctypes.data if a.size else None, YOLO_LAYOUT[layout], F, N, p, dets.ctypes.data, cap, C.byref(n)))
        out = dets[:min(n.value, cap)].copy()
        return (out, n.value) if return_count else out

    def yolodec_device(self, d_tensors, tensor_pitch_bytes, n_tensors, layout, num_fields, num_candidates, params, max_dets=None, return_counts=False):
        """One record array per device tensor d_tensors + i * tensor_pitch_bytes; params: one triple per tensor. One synchronisation."""
        cap = num_candidates if max_dets is None else max_dets
        p, n_p = _yolo_params(params)
        if n_p != n_tensors:
            raise ValueError("yolodec_device: one settings triple per tensor")
        dets = np.zeros(max(n_tensors * cap, 1), YOLO_DET)
        n = (C.c_uint32 * max(n_tensors, 1))()
        self._ck(self.L.mi355_yolodec_tensors_device(self.h, d_tensors, tensor_pitch_bytes, n_tensors, YOLO_LAYOUT[layout], num_fields, num_candidates, p,
                                                     dets.ctypes.data, cap, n))
        out = [dets[t * cap:t * cap + min(n[t], cap)].copy() for t in range(n_tensors)]
        return (out, [n[t] for t in range(n_tensors)]) if return_counts else out

    # ---- yoloxinference's head decode and input tensor (analytics/burn/src/yoloxinference: yolox_burn/model/head.rs, imp.rs)
    def yolox_head_decode_device(self, levels, n_tensors, num_classes, d_out, out_pitch_bytes):
        """The decoded [A, 5 + C] float32 tensor of every head at d_out + i * out_pitch_bytes; levels: YoloxLevel objects or tuples
        (reg, obj, cls, reg_pitch, obj_pitch, cls_pitch, h, w, stride) of device pointers. One launch, asynchronous."""
        self._ck(self.L.mi355_yolox_head_decode_device(self.h, _yolox_levels(levels), len(levels), n_tensors, num_classes, d_out, out_pitch_bytes))

    def yolox_head_dets_device(self, levels, n_tensors, num_classes, params, max_dets=None, return_counts=False):
        """One YOLO_DET record array per head, straight from the device head maps (levels as above); params: one
        (box_thr, class_thr, iou_thr) triple per tensor. max_dets: default A, never truncated. One synchronisation."""
        cap = yolox_candidates(levels) if max_dets is None else max_dets
        p, n_p = _yolo_params(params)
        if n_p != n_tensors:
            raise ValueError("yolox_head_dets_device: one settings triple per tensor")
        dets = np.zeros(max(n_tensors * cap, 1), YOLO_DET)
        n = (C.c_uint32 * max(n_tensors, 1))()
        self._ck(self.L.mi355_yolox_head_dets_device(self.h, _yolox_levels(levels), len(levels), n_tensors, num_classes, p, dets.ctypes.data, cap, n))
        out = [dets[t * cap:t * cap + min(n[t], cap)].copy() for t in range(n_tensors)]
        return (out, [n[t] for t in range(n_tensors)]) if return_counts else out

    def yolox_head_dets(self, levels, params, max_dets=None, return_count=False):
        """The kept boxes of one head held in host memory; levels: (reg, obj, cls, stride) per level, float32 arrays of shape
        (4, h, w), (1, h, w) or (h, w), and (C, h, w); params: (box_thr, class_thr, iou_thr)."""
        keep, lv, C_ = [], [], None
        for reg, obj, cls, stride in levels:
            reg, obj, cls = (np.ascontiguousarray(a, dtype=np.float32) for a in (reg, obj, cls))
            h, w = reg.shape[-2:]
            if reg.shape != (4, h, w) or obj.size != h * w or cls.ndim != 3 or cls.shape[1:] != (h, w) or C_ not in (None, cls.shape[0]):
                raise ValueError("yolox_head_dets: reg (4, h, w), obj (1, h, w), cls (C, h, w) per level, one C")
            C_ = cls.shape[0]
            keep += [reg, obj, cls]
            lv.append(YoloxLevel(reg.ctypes.data, obj.ctypes.data, cls.ctypes.data, 0, 0, 0, h, w, stride, 0))
        cap = yolox_candidates(lv) if max_dets is None else max_dets
        p, _ = _yolo_params(params)
        dets = np.zeros(max(cap, 1), YOLO_DET)
        n = C.c_uint32(0)
        self._ck(self.L.mi355_yolox_head_dets(self.h, _yolox_levels(lv), len(lv), C_ or 0, p, dets.ctypes.data, cap, C.byref(n)))
        out = dets[:min(n.value, cap)].copy()
        return (out, n.value) if return_count else out

    def yolox_input_frames_device(self, d_frames, frame_pitch, stride, n_frames, width, height, d_out, out_pitch_bytes):
        """RGB u8 frames (row stride `stride`, frame i at d_frames + i * frame_pitch) -> [3][H][W] float32 per frame at
        d_out + i * out_pitch_bytes, unscaled. One launch, asynchronous."""
        self._ck(self.L.mi355_yolox_input_frames_device(self.h, d_frames, frame_pitch, stride, n_frames, width, height, d_out, out_pitch_bytes))

    def selftest_yolox_net_op(self, **fields):
        """mi355_selftest_yolox_net_op_device (test only): one op of the network on caller views; kind: a YOLOX_OP name."""
        op = YoloxNetOp()
        fields["kind"] = YOLOX_OP[fields["kind"]]
        for k, v in fields.items():
            setattr(op, k, v)
        self._ck(self.L.mi355_selftest_yolox_net_op_device(self.h, C.byref(op)))

    def selftest_yolox_net_op_bf16(self, **fields):
        """mi355_selftest_yolox_net_op_bf16_device (test only): a dense conv ("conv") or the Focus stem ("focus") as a BF16 net runs it;
        weight is f32 on the device."""
        op = YoloxNetOp()
        fields["kind"] = YOLOX_OP[fields["kind"]]
        for k, v in fields.items():
            setattr(op, k, v)
        self._ck(self.L.mi355_selftest_yolox_net_op_bf16_device(self.h, C.byref(op)))

    # ---- handdetectiontensordec / handlandmarktensordec (analytics/analytics/src/hand)
    def handdec_palm(self, tensor, params, return_count=False):
        """The selected hands of one host palm tensor ([N, 8] float32 rows score, cx, cy, size, kp0x, kp0y, kp2x, kp2y) as a HAND_DET
        record array, in output order. params: (confidence_thr, nms_iou_thr, max_hands[, frame_width, frame_height])."""
        a = np.ascontiguousarray(tensor, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != 8:
            raise ValueError("handdec_palm: a [N, 8] tensor")
        p, _ = _hand_params(params)
        dets = np.zeros(HAND_MAX, HAND_DET)
        n = C.c_uint32(0)
        self._ck(self.L.mi355_handdec_palm_tensor(self.h, a.ctypes.data if a.size else None, a.shape[0], p, dets.ctypes.data, C.byref(n)))
        out = dets[:n.value].copy()
        return (out, n.value) if return_count else out

    def handdec_palm_device(self, d_tensors, tensor_pitch_bytes, n_tensors, num_rows, params, return_counts=False):
        """One HAND_DET record array per device tensor d_tensors + i * tensor_pitch_bytes; params: one tuple per tensor. One launch,
        one synchronisation."""
        p, n_p = _hand_params(params)
        if n_p != n_tensors:
            raise ValueError("handdec_palm_device: one params tuple per tensor")
        dets = np.zeros(max(n_tensors, 1) * HAND_MAX, HAND_DET)
        n = (C.c_uint32 * max(n_tensors, 1))()
        self._ck(self.L.mi355_handdec_palm_tensors_device(self.h, d_tensors, tensor_pitch_bytes, n_tensors, num_rows, p, dets.ctypes.data, n))
        out = [dets[t * HAND_MAX:t * HAND_MAX + n[t]].copy() for t in range(n_tensors)]
        return (out, [n[t] for t in range(n_tensors)]) if return_counts else out

    def handdec_landmarks(self, tensor, params, scores=None):
        """(HAND_DET records, HAND_KP records) of one host landmark tensor ([H, 21 * D] float32, D >= 2), in output order; scores: the
        optional hand score vector (hand i has confidence scores[i] if there is one, else 1.0)."""
        a = np.ascontiguousarray(tensor, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] % 21 != 0:
            raise ValueError("handdec_landmarks: a [H, 21 * D] tensor")
        sc = None if scores is None else np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
        p, _ = _hand_params(params)
        dets, kps = np.zeros(HAND_MAX, HAND_DET), np.zeros(HAND_MAX, HAND_KP)
        n = C.c_uint32(0)
        self._ck(self.L.mi355_handdec_landmarks_tensor(self.h, a.ctypes.data if a.size else None, a.shape[0], a.shape[1] // 21,
                                                       sc.ctypes.data if sc is not None and sc.size else None, 0 if sc is None else sc.size, p, dets.ctypes.data,
                                                       kps.ctypes.data, C.byref(n)))
        return dets[:n.value].copy(), kps[:n.value].copy()

    def handdec_landmarks_device(self, d_landmarks, tensor_pitch_bytes, n_tensors, num_hands, kps_dim, params, d_scores=None, score_pitch_bytes=0, num_scores=0):
        """One (HAND_DET records, HAND_KP records) pair per device tensor d_landmarks + i * tensor_pitch_bytes; params: one tuple per
        tensor; d_scores: null or num_scores scores per tensor at d_scores + i * score_pitch_bytes. One launch, one synchronisation."""
        p, n_p = _hand_params(params)
        if n_p != n_tensors:
            raise ValueError("handdec_landmarks_device: one params tuple per tensor")
        dets, kps = np.zeros(max(n_tensors, 1) * HAND_MAX, HAND_DET), np.zeros(max(n_tensors, 1) * HAND_MAX, HAND_KP)
        n = (C.c_uint32 * max(n_tensors, 1))()
        self._ck(self.L.mi355_handdec_landmarks_tensors_device(self.h, d_landmarks, tensor_pitch_bytes, n_tensors, num_hands, kps_dim, d_scores, score_pitch_bytes,
                                                               num_scores, p, dets.ctypes.data, kps.ctypes.data, n))
        return [(dets[t * HAND_MAX:t * HAND_MAX + n[t]].copy(), kps[t * HAND_MAX:t * HAND_MAX + n[t]].copy()) for t in range(n_tensors)]

    # ---- rsaudioecho
    def echo_setup(self, ring_len):
        self._ck(self.L.mi355_echo_setup(self.h, ring_len))

    def echo_reset(self):
        self._ck(self.L.mi355_echo_reset(self.h))

    def echo_process(self, data, delay_samples, intensity, feedback):
        fn = self.L.mi355_echo_process_f64 if data.dtype == np.float64 else self.L.mi355_echo_process_f32
        assert data.dtype in (np.float32, np.float64) and data.flags.c_contiguous
        self._ck(fn(self.h, data.ctypes.data, data.size, delay_samples, float(intensity), float(feedback)))
        return data

    def echo_state(self, ring_len, stream=0):
        ring = np.zeros(max(ring_len, 1), np.float64)
        pos = C.c_size_t(0)
        self._ck(self.L.mi355_echo_get_state_batch(self.h, stream, ring.ctypes.data, ring_len, C.byref(pos)))
        return ring, pos.value

    def echo_setup_batch(self, n_streams, ring_len):
        self._ck(self.L.mi355_echo_setup_batch(self.h, n_streams, ring_len))

    def echo_process_batch_device(self, dptr, stream_stride, n, is_f64, delay_samples, intensity, feedback):
        """n_streams slices of n samples, stream_stride elements apart, in place in device memory; per-stream parameter lists."""
        d = np.ascontiguousarray(delay_samples, dtype=np.uint64)
        a = np.ascontiguousarray(intensity, dtype=np.float64)
        f = np.ascontiguousarray(feedback, dtype=np.float64)
        self._ck(self.L.mi355_echo_process_batch_device(self.h, dptr, stream_stride, n, int(is_f64), d.ctypes.data, a.ctypes.data, f.ctypes.data))


    # ---- ebur128 (loudness meter)
    _EB_FMT = {np.dtype(np.int16): 0, np.dtype(np.int32): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}

    def ebur128_setup(self, channels, rate, mode=63, channel_class=None):
        cc = None
        if channel_class is not None:
            cc = (C.c_int * channels)(*[int(v) for v in channel_class])
        self._ck(self.L.mi355_ebur128_setup(self.h, channels, rate, mode, cc))
        self._eb_channels = channels

    def ebur128_reset(self):
        self._ck(self.L.mi355_ebur128_reset(self.h))

    # batch of n_streams meters of one configuration, fed in lock step
    def ebur128_setup_batch(self, n_streams, channels, rate, mode=63, channel_class=None):
        cc = None
        if channel_class is not None:
            cc = (C.c_int * channels)(*[int(v) for v in channel_class])
        self._ck(self.L.mi355_ebur128_setup_batch(self.h, n_streams, channels, rate, mode, cc))
        self._eb_channels, self._eb_streams = channels, n_streams

    def ebur128_add_frames_batch(self, data):
        """data: (n_streams, frames, channels) array."""
        a = np.ascontiguousarray(data)
        assert a.ndim == 3 and a.shape[0] == self._eb_streams and a.shape[2] == self._eb_channels
        self._ck(self.L.mi355_ebur128_add_frames_batch(self.h, a.ctypes.data, a.shape[1], self._EB_FMT[a.dtype]))

    def ebur128_add_frames_batch_device(self, d_ptr, frames, fmt):
        self._ck(self.L.mi355_ebur128_add_frames_batch_device(self.h, d_ptr, frames, fmt))

    def ebur128_loudness_batch(self, what):
        out = (C.c_double * self._eb_streams)()
        self._ck(self.L.mi355_ebur128_loudness_batch(self.h, what, out))
        return np.array(out)

    def ebur128_peak_batch(self, true_peak=False):
        out = (C.c_double * (self._eb_streams * self._eb_channels))()
        self._ck(self.L.mi355_ebur128_peak_batch(self.h, int(true_peak), out))
        return np.array(out).reshape(self._eb_streams, self._eb_channels)

    def ebur128_add_frames(self, data, planar=False):
        a = np.ascontiguousarray(data)
        fmt = self._EB_FMT[a.dtype]
        if planar:
            frames = a.shape[1]
            ptrs = (C.c_void_p * a.shape[0])(*[a[c].ctypes.data for c in range(a.shape[0])])
            self._ck(self.L.mi355_ebur128_add_frames_planar(self.h, ptrs, frames, fmt))
        else:
            self._ck(self.L.mi355_ebur128_add_frames(self.h, a.ctypes.data, a.size // self._eb_channels, fmt))

    def _eb_get(self, name):
        v = C.c_double(0)
        self._ck(getattr(self.L, name)(self.h, C.byref(v)))
        return v.value

    def ebur128_loudness_momentary(self):
        return self._eb_get("mi355_ebur128_loudness_momentary")

    def ebur128_loudness_shortterm(self):
        return self._eb_get("mi355_ebur128_loudness_shortterm")

    def ebur128_loudness_global(self):
        return self._eb_get("mi355_ebur128_loudness_global")

    def ebur128_relative_threshold(self):
        return self._eb_get("mi355_ebur128_relative_threshold")

    def ebur128_loudness_range(self):
        return self._eb_get("mi355_ebur128_loudness_range")

    def ebur128_sample_peak(self, c):
        v = C.c_double(0)
        self._ck(self.L.mi355_ebur128_sample_peak(self.h, c, C.byref(v)))
        return v.value

    def ebur128_true_peak(self, c):
        v = C.c_double(0)
        self._ck(self.L.mi355_ebur128_true_peak(self.h, c, C.byref(v)))
        return v.value


def warm_clocks(fn, sync, seconds=0.25):
    """Untimed preamble for microbenchmarks: run fn() for `seconds` so that the GPU has left its idle clocks (the first
    ~20 ms of work after idling run 15-20 % slower on MI355X)."""
    import time as _t
    t_end = _t.perf_counter() + seconds
    while _t.perf_counter() < t_end:
        for _ in range(8):
            fn()
        sync()
