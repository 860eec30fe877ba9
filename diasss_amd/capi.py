"""ctypes binding of libdsss.so (the C ABI declared in include/dsss.h).

This is the only way Python reaches the hot path: there is no Python or CPU implementation behind it.
If the HIP library has not been built, or no MI355X is visible, loading/creating fails loudly.
"""
import ctypes as C
import os
import subprocess
import sys
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DSSS_LIB", os.path.join(_HERE, "libdsss.so"))     # DSSS_LIB: A/B runs of two builds on one box
_LIB = None
_HIP = None

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4")])
LC_DTYPE = np.dtype([("rel", "<f8", (12,)), ("var", "<f8", (6,)), ("score", "<f8"), ("iters", "<i4"),
                     ("_pad", "<i4"), ("err0", "<f8"), ("err1", "<f8")])
LCEDGE_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("rel", "<f8", (12,)), ("var", "<f8", (6,))])

K_NAMES = ["row_reduce", "pre_misc", "normalize", "pyramid", "fast", "fast_compact", "desc", "filter", "match", "scc", "rows", "lc", "pg",
           "quadtree", "pg_acc", "pg_diag", "pg_trsm", "pg_bwd", "pg_subtree", "pg_asm", "pg_comm", "pg_rsu", "match_done", "sift"]


class MaskParams(C.Structure):
    _fields_ = [("factor", C.c_double), ("width", C.c_int32), ("r", C.c_int32), ("side", C.c_int32)]


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale", C.c_float), ("nlevels", C.c_int32),
                ("ini_th", C.c_int32), ("min_th", C.c_int32), ("descriptor", C.c_int32)]


DESC_ORB, DESC_SIFT128 = 0, 1          # include/dsss.h DSSS_DESC_*


class MatchParams(C.Structure):
    _fields_ = [("use_l2", C.c_int32), ("radius", C.c_double), ("bound_same", C.c_int32), ("bound_diff", C.c_int32),
                ("l2_bound", C.c_double), ("ratio", C.c_double), ("scc_iters", C.c_int32), ("pix_err", C.c_double),
                ("merge_thr", C.c_double)]


class PGParams(C.Structure):
    _fields_ = [("max_iters", C.c_int32), ("rel_tol", C.c_double), ("abs_tol", C.c_double), ("lambda0", C.c_double),
                ("lambda_factor", C.c_double), ("lambda_max", C.c_double), ("min_fidelity", C.c_double),
                ("add_noise", C.c_int32)]


class MosaicParams(C.Structure):
    """dsss_mosaic_params: cell (ix, iy) covers [x0 + ix cell, x0 + (ix + 1) cell) x [y0 + iy cell, ...); layers are H x W"""
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("cell", C.c_double), ("W", C.c_int32), ("H", C.c_int32),
                ("use_mask", C.c_int32), ("pad_", C.c_int32)]


class GainParams(C.Structure):
    """dsss_gain_params: the fewest samples a column (with its window) needs to get a gain of its own, the half-width of the window
    in columns (0..16, never across the nadir) and the grey level the columns are brought to (0: the pooled mean)"""
    _fields_ = [("min_count", C.c_int32), ("smooth", C.c_int32), ("target", C.c_int32), ("pad_", C.c_int32)]


class GainBands(C.Structure):
    """dsss_gain_bands: nbands (1..16) altitude bands of width dalt from alt0; the band of an altitude a is floor((a - alt0) / dalt),
    held to [0, nbands - 1] (NaN and everything below alt0: band 0)"""
    _fields_ = [("alt0", C.c_double), ("dalt", C.c_double), ("nbands", C.c_int32), ("pad_", C.c_int32)]


def _bands(bands):
    """a GainBands, or (alt0, dalt, nbands) -> GainBands"""
    return bands if isinstance(bands, GainBands) else GainBands(float(bands[0]), float(bands[1]), int(bands[2]), 0)


class CompParams(C.Structure):
    """dsss_comp_params: the priority a cell's winner is chosen by (COMP_NEAR, COMP_FAR, COMP_MID, COMP_FIRST) and the radius, in cells
    (0..4, 0: none), within which enclosed holes are filled"""
    _fields_ = [("mode", C.c_int32), ("fill_radius", C.c_int32)]


class CompInfo(C.Structure):
    """dsss_comp_info: the cells that hold a sample, the cells filled and the cells left empty; they sum to W H"""
    _fields_ = [("direct", C.c_int64), ("filled", C.c_int64), ("empty", C.c_int64)]


class FootprintParams(C.Structure):
    """dsss_footprint_params: the most sub-samples of a sample along each of its two steps (1..8; 1: point samples) and the longest
    step, in metres, that is bridged (finite, > 0).  The library's defaults are 4 and 1.0 (footprint_params_default)"""
    _fields_ = [("max_steps", C.c_int32), ("pad_", C.c_int32), ("max_gap", C.c_double)]


def _footprint(footprint):
    """None (the library's defaults), a FootprintParams, or (max_steps, max_gap) -> what goes to the C argument"""
    if footprint is None or isinstance(footprint, FootprintParams):
        return footprint
    return FootprintParams(int(footprint[0]), 0, float(footprint[1]))


class CanvasParams(C.Structure):
    """dsss_canvas_params (include/dsss_canvas.h): footprint 0 = point samples, move = CANVAS_MOVE_AUTO or CANVAS_MOVE_SPLIT, fp = the
    footprint parameters of a footprint canvas"""
    _fields_ = [("footprint", C.c_int32), ("move", C.c_int32), ("fp", FootprintParams)]


class CanvasPutInfo(C.Structure):
    """dsss_canvas_put_info: frames added, moved and skipped by a put, the workgroups it launched and the window (ox, oy, bw, bh; bw = 0:
    none) it touched"""
    _fields_ = [("added", C.c_int32), ("moved", C.c_int32), ("skipped", C.c_int32), ("pad_", C.c_int32), ("pings", C.c_int64), ("win", C.c_int32 * 4)]


CANVAS_MOVE_AUTO, CANVAS_MOVE_SPLIT = 0, 1                        # include/dsss_canvas.h DSSS_CANVAS_MOVE_*


class PingStat(C.Structure):
    """dsss_ping_stat (include/dsss_profile.h): one ping of a profiled frame, [0] port and [1] starboard: the binned samples, the samples
    compared against the mosaic of the other frames, and sum |d|, sum d^2 and sum d of their differences"""
    _fields_ = [("binned", C.c_uint32 * 2), ("n", C.c_uint32 * 2), ("sad", C.c_uint32 * 2), ("ssd", C.c_uint32 * 2), ("sd", C.c_int32 * 2)]


class ProfileParams(C.Structure):
    """dsss_profile_params: the fewest samples of other frames a cell needs for a sample in it to be compared (1..2^24)"""
    _fields_ = [("min_count", C.c_int32), ("pad_", C.c_int32)]


class ProfileInfo(C.Structure):
    """dsss_profile_info: the records of a call summed, and rms = n ? sqrt(ssd / n) : 0"""
    _fields_ = [("pings", C.c_int64), ("binned", C.c_int64), ("n", C.c_int64), ("sad", C.c_int64), ("ssd", C.c_int64), ("sd", C.c_int64), ("rms", C.c_double)]


assert C.sizeof(PingStat) == 40 and C.sizeof(ProfileParams) == 8 and C.sizeof(ProfileInfo) == 56
PING_DTYPE = np.dtype(PingStat)          # the rows Context.profile_mosaic and Canvas.profile return: ten integers, five fields of (port, starboard)
PROFILE_NONE = -32768                    # include/dsss_profile.h DSSS_PROFILE_NONE: a sample of a residual layer that is not compared
PROFILE_OUTPUTS = ("stats", "diff", "info")
COMP_NEAR, COMP_FAR, COMP_MID, COMP_FIRST = 0, 1, 2, 3          # include/dsss.h DSSS_COMP_*
COMP_MODES = {"near": COMP_NEAR, "far": COMP_FAR, "mid": COMP_MID, "first": COMP_FIRST}
COMP_LAYERS = (("img", np.uint8), ("src_frame", np.int32), ("src_ping", np.int32), ("src_col", np.int32), ("fill", np.uint8))   # in the order of the C arguments


class RegParams(C.Structure):
    """dsss_reg_params: search radius in cells (0..16) and the fewest overlapping cells a shift needs to be usable"""
    _fields_ = [("radius", C.c_int32), ("min_cells", C.c_int32)]


class RegResult(C.Structure):
    """dsss_reg_result: peak shift in cells, offset in metres (sub-cell), ZNCC and overlapping cells at the peak and at zero shift,
    on_border = 1 when the peak lies on the border of the search square"""
    _fields_ = [("dx", C.c_int32), ("dy", C.c_int32), ("off_x", C.c_double), ("off_y", C.c_double), ("zncc", C.c_double),
                ("zncc0", C.c_double), ("n", C.c_int64), ("n0", C.c_int64), ("on_border", C.c_int32), ("pad_", C.c_int32)]


REG_DTYPE = np.dtype(RegResult)          # the rows Context.mosaic_register returns


class RegCallInfo(C.Structure):
    """dsss_reg_call_info: what the last registration call of a context that succeeded did: tables scored by mosaic_peak_kernel / by
    the host, bytes it copied device -> host, stream synchronisations it made"""
    _fields_ = [("tables_device", C.c_int64), ("tables_host", C.c_int64), ("bytes_down", C.c_int64), ("syncs", C.c_int64)]


class RegSeg(C.Structure):
    """dsss_reg_seg: one (pair, segment) row of the registration by segments: pair = index into the pair list, pings [p0, p1) of the
    pair's frame b, r = the RegResult of the segment's table, sx, sy = sum of ix, iy over the overlapping cells at the peak shift"""
    _fields_ = [("pair", C.c_int32), ("seg", C.c_int32), ("p0", C.c_int32), ("p1", C.c_int32), ("r", RegResult),
                ("sx", C.c_int64), ("sy", C.c_int64)]


REGSEG_DTYPE = np.dtype(RegSeg)          # the rows Context.mosaic_register_segments returns (field "r" is a REG_DTYPE record)


class RegEdgeParams(C.Structure):
    """dsss_reg_edge_params: the lowest ZNCC of an accepted segment, sigma of the offset in cells, of the height (m), of the rotation (rad)"""
    _fields_ = [("min_zncc", C.c_double), ("sigma_xy_cells", C.c_double), ("sigma_z", C.c_double), ("sigma_rot", C.c_double)]


class RegYawParams(C.Structure):
    """dsss_reg_yaw_params: the fan of rotations a segment is registered under: nyaw angles (odd, 1..17), step radians apart, about 0"""
    _fields_ = [("nyaw", C.c_int32), ("pad_", C.c_int32), ("step", C.c_double)]


class RegSegYaw(C.Structure):
    """dsss_reg_seg_yaw: s = the RegSeg of the chosen angle k, yaw_on_border = 1 when k is the first or the last angle of the fan, theta =
    the chosen angle, theta_hat = the angle refined by a parabola through the neighbours' ZNCC, zncc_k0 = the peak ZNCC without rotation"""
    _fields_ = [("s", RegSeg), ("k", C.c_int32), ("yaw_on_border", C.c_int32), ("theta", C.c_double), ("theta_hat", C.c_double),
                ("zncc_k0", C.c_double)]


REGSEGYAW_DTYPE = np.dtype(RegSegYaw)    # the rows Context.mosaic_register_segments_yaw returns (field "s" is a REGSEG_DTYPE record)


class RegEdgeYawParams(C.Structure):
    """dsss_reg_edge_yaw_params: e = the RegEdgeParams, fan = the fan the rows were registered with, sigma of the yaw in steps of the fan"""
    _fields_ = [("e", RegEdgeParams), ("fan", RegYawParams), ("sigma_yaw_steps", C.c_double)]


class RegPyrParams(C.Structure):
    """dsss_reg_pyr_params: the cell pyramid a segment is registered over: levels (1..4; 1 = the flat registration), and the radius in
    cells of the refinement below the top level (1..16)"""
    _fields_ = [("levels", C.c_int32), ("refine", C.c_int32)]


class RegSegPyr(C.Structure):
    """dsss_reg_seg_pyr: s = the RegSeg of the finest level with a usable peak (on_border = 1 unless the row finished at level 0 away from
    every border), level = that level (-1: none), border_mask = bit l set when level l's peak lay on the border of its square,
    lx, ly, lz = the total shift in cells of level l and the peak ZNCC per level (0, 0, -2: not reached)"""
    _fields_ = [("s", RegSeg), ("level", C.c_int32), ("border_mask", C.c_int32), ("lx", C.c_int32 * 4), ("ly", C.c_int32 * 4), ("lz", C.c_double * 4)]


REGSEGPYR_DTYPE = np.dtype(RegSegPyr)    # the rows Context.mosaic_register_segments_pyr returns (field "s" is a REGSEG_DTYPE record)


class PGGateParams(C.Structure):
    """dsss_pg_gate_params: chi-square gate, the factor between the worst kept edge and the threshold of a round, solves at most"""
    _fields_ = [("gate", C.c_double), ("decade", C.c_double), ("max_solves", C.c_int32), ("pad_", C.c_int32)]


class DsssError(RuntimeError):
    code = None          # the DSSS_E_* value where the error came from the library


# dsss_raw_type: the element type of a raw waterfall
RAW_F64, RAW_F32, RAW_U16, RAW_U8 = 0, 1, 2, 3
_RAW_SIZE = {RAW_F64: 8, RAW_F32: 4, RAW_U16: 2, RAW_U8: 1}
_RAW_OF_DTYPE = {"float64": RAW_F64, "float32": RAW_F32, "uint16": RAW_U16, "uint8": RAW_U8}


def raw_type_of(a, raw_type=None):
    """dsss_raw_type of a waterfall (numpy array or torch tensor), from its dtype.  torch has no uint16 arithmetic on every build: a
    u16 image may come as a tensor whose storage is viewed as int16, with raw_type=RAW_U16 given explicitly (an explicit type must
    have the element size of the array's dtype).  Any dtype but uint8, uint16, float32, float64 raises TypeError."""
    name = str(a.dtype).replace("torch.", "")
    if raw_type is None:
        if name not in _RAW_OF_DTYPE:
            raise TypeError("raw waterfall of dtype %s: uint8, uint16, float32 or float64 expected" % name)
        return _RAW_OF_DTYPE[name]
    raw_type = int(raw_type)
    itemsize = a.dtype.itemsize if isinstance(a, np.ndarray) else a.element_size()
    if _RAW_SIZE.get(raw_type) != itemsize:
        raise TypeError("raw_type %d does not have the element size of dtype %s" % (raw_type, name))
    return raw_type


class FramesArgs:
    """argument arrays of dsss_frames_set_typed (see Context.frames_args)"""

    def __init__(self, ids, raws, Ns, Ms, poses, alts, grs, raw_types=None):
        n = self.n = len(ids)
        if not (len(raws) == len(Ns) == len(Ms) == len(poses) == len(alts) == len(grs) == n) or (raw_types is not None and len(raw_types) != n):
            raise ValueError("frames_set: the per-frame lists differ in length")
        _torch = sys.modules.get("torch")                      # (only a caller that has torch can hand tensors over)
        # the type of every image from its own dtype (a list may mix them), or as given
        self.raw_type = np.fromiter((RAW_F64 if a is None else raw_type_of(a, None if raw_types is None else raw_types[i])
                                     for i, a in enumerate(raws)), np.int32, n)

        def addr(a, what, shape=None, typed=False):
            if a is None:
                return 0
            if typed:                                          # a raw image: its dtype was checked above
                if not (a.flags.c_contiguous if isinstance(a, np.ndarray) else a.is_contiguous()):
                    raise TypeError("frames_set: %s must be contiguous" % what)
                if shape is not None and tuple(a.shape) != shape:
                    raise ValueError("frames_set: %s has shape %s, expected %s" % (what, tuple(a.shape), shape))
                return a.__array_interface__["data"][0] if isinstance(a, np.ndarray) else a.data_ptr()
            if isinstance(a, np.ndarray):
                if a.dtype != np.float64 or not a.flags.c_contiguous:
                    raise TypeError("frames_set: %s must be a C-contiguous float64 array" % what)
                if shape is not None and a.shape != shape:
                    raise ValueError("frames_set: %s has shape %s, expected %s" % (what, a.shape, shape))
                return a.__array_interface__["data"][0]
            if _torch is not None and isinstance(a, _torch.Tensor):
                if a.dtype != _torch.float64 or not a.is_contiguous():
                    raise TypeError("frames_set: %s must be a contiguous float64 tensor" % what)
                if shape is not None and tuple(a.shape) != shape:
                    raise ValueError("frames_set: %s has shape %s, expected %s" % (what, tuple(a.shape), shape))
                return a.data_ptr()                            # host (pinned or pageable) or device: the library asks the runtime which
            raise TypeError("frames_set: %s must be None, a numpy array or a torch tensor" % what)
        self.ids = np.ascontiguousarray(ids, np.int32); self.N = np.ascontiguousarray(Ns, np.int32); self.M = np.ascontiguousarray(Ms, np.int32)
        self.p_raw = np.fromiter((addr(a, "raw[%d]" % i, (int(self.N[i]), int(self.M[i])), True) for i, a in enumerate(raws)), np.uintp, n)
        self.p_pose = np.fromiter((addr(a, "pose[%d]" % i, (int(self.N[i]), 6)) for i, a in enumerate(poses)), np.uintp, n)
        self.p_alt = np.fromiter((addr(a, "alt[%d]" % i, (int(self.N[i]),)) for i, a in enumerate(alts)), np.uintp, n)
        self.p_gr = np.fromiter((addr(a, "grange[%d]" % i, (int(self.M[i]) // 2,)) for i, a in enumerate(grs)), np.uintp, n)
        if (self.p_pose == 0).any() or (self.p_alt == 0).any() or (self.p_gr == 0).any():
            raise ValueError("frames_set: pose, altitude and ground range are required for every frame")
        self.keep = dict(zip(map(int, ids), zip(raws, poses, alts, grs)))      # the arrays stay alive as long as this object (or the Context) does


def build(force=False):
    """compile libdsss.so for gfx950 with hipcc (cross-compiles without a GPU)"""
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", src, "-s", "clean"])
    subprocess.check_call(["make", "-C", src, "-s", "-j4"])
    return LIB_PATH


def _load_hip_runtime():
    """libdsss.so leaves the HIP runtime symbols undefined so that ONE runtime serves the whole process.
    PyTorch ships its own libamdhip64 (soname libamdhip64.so) next to the system one (libamdhip64.so.7); loading
    both makes the second one see no GPU.  So: if torch is importable use the copy it loads, else the system copy."""
    try:
        import torch  # noqa: F401  (loads torch/lib/libamdhip64.so)
        cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            return C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass
    for cand in ("/opt/rocm/lib/libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so"):
        try:
            return C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            continue
    raise DsssError("no HIP runtime (libamdhip64) found")


def lib():
    global _LIB, _HIP
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise DsssError("libdsss.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                            "there is no CPU fallback")
        _HIP = _load_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.dsss_strerror.restype = C.c_char_p
        L.dsss_last_error.restype = C.c_char_p
        L.dsss_last_error.argtypes = [C.c_void_p]
        L.dsss_stream.restype = C.c_void_p
        L.dsss_stream.argtypes = [C.c_void_p]
        L.dsss_features_pack_bytes.restype = C.c_size_t
        L.dsss_features_pack_bytes.argtypes = [C.c_void_p]
        L.dsss_raw_type_size.restype = C.c_size_t
        L.dsss_raw_type_size.argtypes = [C.c_int]
        L.dsss_frame_set_typed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dsss_frames_set_typed.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
        L.dsss_frame_raw_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
        L.dsss_frame_raw_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.dsss_comm_init_callback.argtypes = [C.c_void_p, C.c_int, C.c_int, COMM_FN, C.c_void_p]
        L.dsss_comm_init_device_callback.argtypes = [C.c_void_p, C.c_int, C.c_int, COMM_DEV_FN, C.c_void_p]
        L.dsss_comm_frame_owner.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.dsss_posegraph_edge_report.restype = C.c_int
        L.dsss_posegraph_edge_report.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dsss_pg_gate_params_default.restype = None
        L.dsss_pg_gate_params_default.argtypes = [C.POINTER(PGGateParams)]
        L.dsss_posegraph_solve_gated.restype = C.c_int
        L.dsss_posegraph_solve_gated.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(PGGateParams), C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.dsss_gain_params_default.restype = None
        L.dsss_gain_params_default.argtypes = [C.POINTER(GainParams)]
        L.dsss_mosaic_gain_stats.restype = C.c_int
        L.dsss_mosaic_gain_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.dsss_mosaic_gain_table.restype = C.c_int
        L.dsss_mosaic_gain_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(GainParams), C.c_void_p, C.POINTER(C.c_int32)]
        L.dsss_mosaic_gain_set.restype = C.c_int
        L.dsss_mosaic_gain_set.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.dsss_mosaic_gain_get.restype = C.c_int
        L.dsss_mosaic_gain_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.dsss_gain_band.restype = C.c_int
        L.dsss_gain_band.argtypes = [C.POINTER(GainBands), C.c_double, C.POINTER(C.c_int32)]
        L.dsss_mosaic_gain_stats_banded.restype = C.c_int
        L.dsss_mosaic_gain_stats_banded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(GainBands), C.c_void_p, C.c_void_p]
        L.dsss_mosaic_gain_table_banded.restype = C.c_int
        L.dsss_mosaic_gain_table_banded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(GainParams), C.c_void_p, C.POINTER(C.c_int32)]
        L.dsss_mosaic_gain_set_banded.restype = C.c_int
        L.dsss_mosaic_gain_set_banded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(GainBands)]
        L.dsss_mosaic_gain_get_banded.restype = C.c_int
        L.dsss_mosaic_gain_get_banded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(GainBands)]
        L.dsss_frame_get_corrected.restype = C.c_int
        L.dsss_frame_get_corrected.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.dsss_reg_params_default.restype = None
        L.dsss_comp_params_default.restype = None
        L.dsss_comp_params_default.argtypes = [C.POINTER(CompParams)]
        L.dsss_mosaic_comp_rank.restype = C.c_int
        L.dsss_mosaic_comp_rank.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        L.dsss_mosaic_fill_host.restype = C.c_int
        L.dsss_mosaic_fill_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.dsss_mosaic_composite.restype = C.c_int
        L.dsss_mosaic_composite.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(MosaicParams), C.POINTER(CompParams)] + [C.c_void_p] * 5 + [
            C.POINTER(CompInfo)]
        L.dsss_footprint_params_default.restype = None
        L.dsss_footprint_params_default.argtypes = [C.POINTER(FootprintParams)]
        L.dsss_mosaic_footprint_steps.restype = C.c_int
        L.dsss_mosaic_footprint_steps.argtypes = [C.POINTER(FootprintParams), C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int32)]
        L.dsss_mosaic_render_footprint.restype = C.c_int
        L.dsss_mosaic_render_footprint.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(MosaicParams), C.POINTER(FootprintParams)] + [
            C.c_void_p] * 3
        L.dsss_mosaic_composite_footprint.restype = C.c_int
        L.dsss_mosaic_composite_footprint.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(MosaicParams), C.POINTER(CompParams),
                                                      C.POINTER(FootprintParams)] + [C.c_void_p] * 5 + [C.POINTER(CompInfo)]
        L.dsss_reg_params_default.argtypes = [C.POINTER(RegParams)]
        L.dsss_mosaic_register.restype = C.c_int
        L.dsss_mosaic_register.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(MosaicParams), C.c_void_p, C.c_void_p,
                                           C.c_int, C.POINTER(RegParams), C.c_void_p, C.c_void_p]
        L.dsss_mosaic_register_peak.restype = C.c_int
        L.dsss_mosaic_register_peak.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(RegResult)]
        L.dsss_mosaic_register_segments.restype = C.c_int
        L.dsss_mosaic_register_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(MosaicParams), C.c_void_p, C.c_void_p,
                                                    C.c_int, C.c_int, C.POINTER(RegParams), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]
        L.dsss_reg_edge_params_default.restype = None
        L.dsss_reg_edge_params_default.argtypes = [C.POINTER(RegEdgeParams)]
        L.dsss_register_edge.restype = C.c_int
        L.dsss_register_edge.argtypes = [C.c_void_p, C.POINTER(MosaicParams), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                         C.POINTER(RegEdgeParams), C.c_void_p]
        L.dsss_mosaic_register_edges.restype = C.c_int
        L.dsss_mosaic_register_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(MosaicParams), C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_int, C.POINTER(RegEdgeParams), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.dsss_reg_yaw_params_default.restype = None
        L.dsss_reg_yaw_params_default.argtypes = [C.POINTER(RegYawParams)]
        L.dsss_register_rotate_rows.restype = C.c_int
        L.dsss_register_rotate_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p]
        L.dsss_register_yaw_peak.restype = C.c_int
        L.dsss_register_yaw_peak.argtypes = [C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                             C.POINTER(C.c_double)]
        L.dsss_mosaic_register_segments_yaw.restype = C.c_int
        L.dsss_mosaic_register_segments_yaw.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(MosaicParams), C.c_void_p,
                                                        C.c_void_p, C.c_int, C.c_int, C.POINTER(RegParams), C.POINTER(RegYawParams), C.c_void_p, C.c_int,
                                                        C.POINTER(C.c_int), C.c_void_p]
        L.dsss_reg_edge_yaw_params_default.restype = None
        L.dsss_reg_edge_yaw_params_default.argtypes = [C.POINTER(RegEdgeYawParams)]
        L.dsss_register_edge_yaw.restype = C.c_int
        L.dsss_register_edge_yaw.argtypes = [C.c_void_p, C.POINTER(MosaicParams), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                             C.POINTER(RegEdgeYawParams), C.c_void_p]
        L.dsss_mosaic_register_edges_yaw.restype = C.c_int
        L.dsss_mosaic_register_edges_yaw.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(MosaicParams), C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_int, C.POINTER(RegEdgeYawParams), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.dsss_reg_pyr_params_default.restype = None
        L.dsss_reg_pyr_params_default.argtypes = [C.POINTER(RegPyrParams)]
        L.dsss_register_pyr_step.restype = C.c_int
        L.dsss_register_pyr_step.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(RegResult),
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.dsss_mosaic_register_segments_pyr.restype = C.c_int
        L.dsss_mosaic_register_segments_pyr.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(MosaicParams), C.c_void_p,
                                                        C.c_void_p, C.c_int, C.c_int, C.POINTER(RegParams), C.POINTER(RegPyrParams), C.c_void_p, C.c_int,
                                                        C.POINTER(C.c_int), C.c_void_p]
        L.dsss_mosaic_register_peaks.restype = C.c_int
        L.dsss_mosaic_register_peaks.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_void_p]
        L.dsss_mosaic_register_info.restype = C.c_int
        L.dsss_mosaic_register_info.argtypes = [C.c_void_p, C.POINTER(RegCallInfo)]
        L.dsss_canvas_params_default.restype = None
        L.dsss_canvas_params_default.argtypes = [C.POINTER(CanvasParams)]
        L.dsss_canvas_create.argtypes = [C.c_void_p, C.POINTER(MosaicParams), C.POINTER(CanvasParams), C.POINTER(C.c_void_p)]
        L.dsss_canvas_destroy.argtypes = [C.c_void_p]
        L.dsss_canvas_put.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(CanvasPutInfo)]
        L.dsss_canvas_remove.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.dsss_canvas_clear.argtypes = [C.c_void_p]
        L.dsss_canvas_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dsss_canvas_dirty.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.dsss_canvas_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.dsss_canvas_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.dsss_canvas_frame_window.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        for name in ("create", "destroy", "put", "remove", "clear", "read", "dirty", "frames", "rows", "frame_window"):
            getattr(L, "dsss_canvas_" + name).restype = C.c_int
        L.dsss_profile_params_default.restype = None
        L.dsss_profile_params_default.argtypes = [C.POINTER(ProfileParams)]
        L.dsss_profile_summary.restype = C.c_int
        L.dsss_profile_summary.argtypes = [C.c_void_p, C.c_int64, C.POINTER(ProfileInfo)]
        L.dsss_profile_mosaic.restype = C.c_int
        L.dsss_profile_mosaic.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(MosaicParams), C.c_void_p, C.c_int,
                                          C.POINTER(ProfileParams), C.c_void_p, C.c_void_p, C.POINTER(ProfileInfo)]
        L.dsss_profile_canvas.restype = C.c_int
        L.dsss_profile_canvas.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(ProfileParams), C.c_void_p, C.c_void_p, C.POINTER(ProfileInfo)]
        _LIB = L
    return _LIB


COMM_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t)
COMM_DEV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)


def raw_type_size(raw_type):
    """dsss_raw_type_size: bytes per sample of a dsss_raw_type, 0 for anything else"""
    return int(lib().dsss_raw_type_size(int(raw_type)))


def _ptr(a):
    """host numpy array, torch tensor (host or device) or raw int address -> void*"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags.c_contiguous
        return C.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):
        assert a.is_contiguous()
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(int(a))


def mosaic_grid(bbox4, cell):
    """dsss_mosaic_grid: the MosaicParams of the grid that covers bbox4 = (xmin, xmax, ymin, ymax) with cells of edge `cell` (use_mask = 1).
    Host arithmetic, no context."""
    bb = np.ascontiguousarray(bbox4, np.float64); assert bb.shape == (4,)
    p = MosaicParams()
    L = lib()
    rc = L.dsss_mosaic_grid(_ptr(bb), C.c_double(cell), C.byref(p))
    if rc != 0:
        e = DsssError("dsss_mosaic_grid: %s (bbox %s, cell %r)" % (L.dsss_strerror(rc).decode(), bb.tolist(), cell))
        e.code = rc
        raise e
    return p


def gain_params_default():
    g = GainParams(); lib().dsss_gain_params_default(C.byref(g)); return g


def gain_band(bands, alt):
    """dsss_gain_band: the band of the altitude `alt` under `bands` (a GainBands or (alt0, dalt, nbands)).  Host arithmetic, no context."""
    L = lib()
    b = C.c_int32(-1)
    rc = L.dsss_gain_band(C.byref(_bands(bands)) if bands is not None else None, C.c_double(alt), C.byref(b))
    if rc != 0:
        e = DsssError("dsss_gain_band: %s" % L.dsss_strerror(rc).decode())
        e.code = rc
        raise e
    return int(b.value)


def mosaic_gain_table(sum, cnt, params=None, nbands=None):
    """dsss_mosaic_gain_table: the column statistics S, C (M uint64 each, as Context.mosaic_gain_stats returns them) -> (gain, T): the
    range-gain table (M uint16, Q8) and the grey level it brings the columns to.  params: a GainParams, None = the defaults.
    nbands: dsss_mosaic_gain_table_banded on S, C of nbands x M (as mosaic_gain_stats(..., bands=) returns them) -> (gain nbands x M, T).
    Host arithmetic, no context."""
    L = lib()
    if sum is not None:
        sum = np.ascontiguousarray(sum, np.uint64)
    if cnt is not None:
        cnt = np.ascontiguousarray(cnt, np.uint64)
    if sum is not None and cnt is not None and sum.shape != cnt.shape:
        raise ValueError("mosaic_gain_table: %d sums and %d counts" % (sum.size, cnt.size))
    first = sum if sum is not None else cnt
    T = C.c_int32(0)
    pp = C.byref(params) if params is not None else None
    if nbands is None:
        M = len(first) if first is not None else 0
        gain = np.empty(max(M, 0), np.uint16)
        rc = L.dsss_mosaic_gain_table(_ptr(sum), _ptr(cnt), int(M), pp, _ptr(gain), C.byref(T))
        name = "dsss_mosaic_gain_table"
    else:
        M = first.shape[-1] if first is not None and first.ndim == 2 else 0
        if first is not None and first.shape != (int(nbands), M):
            raise ValueError("mosaic_gain_table: statistics of shape %s for %d bands" % (first.shape, nbands))
        gain = np.empty((max(int(nbands), 0), M), np.uint16)
        rc = L.dsss_mosaic_gain_table_banded(_ptr(sum), _ptr(cnt), int(M), int(nbands), pp, _ptr(gain), C.byref(T))
        name = "dsss_mosaic_gain_table_banded"
    if rc != 0:
        e = DsssError("%s: %s (M %d)" % (name, L.dsss_strerror(rc).decode(), M))
        e.code = rc
        raise e
    return gain, int(T.value)


def comp_params_default():
    p = CompParams(); lib().dsss_comp_params_default(C.byref(p)); return p


def mosaic_comp_rank(mode, M, col):
    """dsss_mosaic_comp_rank: the priority rank q (smaller wins) of column col of a frame of M columns under `mode` (a COMP_* value or
    its name).  Host arithmetic, no context."""
    L = lib()
    q = C.c_int32(-1)
    rc = L.dsss_mosaic_comp_rank(int(COMP_MODES.get(mode, mode)), int(M), int(col), C.byref(q))
    if rc != 0:
        raise _host_error(L, "dsss_mosaic_comp_rank", rc)
    return int(q.value)


def mosaic_fill_host(valid, R):
    """dsss_mosaic_fill_host: the gap-fill rule on a layer of validity flags (H x W, != 0: the cell holds a sample) -> (donor, fill):
    donor (int32, H x W) = the cell index iy W + ix each cell takes its value from (its own where it holds a sample, -1 where it stays
    empty), fill (uint8) = 0, the donor's dx^2 + dy^2, or 255.  Host arithmetic, no context."""
    L = lib()
    valid = np.ascontiguousarray(valid, np.uint8); assert valid.ndim == 2
    H, W = valid.shape
    donor = np.empty((H, W), np.int32); fill = np.empty((H, W), np.uint8)
    rc = L.dsss_mosaic_fill_host(_ptr(valid), int(W), int(H), int(R), _ptr(donor), _ptr(fill))
    if rc != 0:
        raise _host_error(L, "dsss_mosaic_fill_host", rc)
    return donor, fill


def footprint_params_default():
    p = FootprintParams(); lib().dsss_footprint_params_default(C.byref(p)); return p


def profile_params_default():
    p = ProfileParams(); lib().dsss_profile_params_default(C.byref(p)); return p


def profile_summary(stats):
    """dsss_profile_summary: rows of PING_DTYPE -> their ProfileInfo (host arithmetic)"""
    stats = np.ascontiguousarray(stats, PING_DTYPE)
    info = ProfileInfo()
    rc = lib().dsss_profile_summary(_ptr(stats) if len(stats) else None, len(stats), C.byref(info))
    if rc:
        raise _host_error(lib(), "dsss_profile_summary", rc)
    return info


def _profile_outputs(sizes, want):
    """the host arrays of a profile call over frames of `sizes` = [(N, M), ...] -> (stats, diff, info), None where not in `want`"""
    for w in want:
        if w not in PROFILE_OUTPUTS:
            raise ValueError("profile: no output %r (%s)" % (w, ", ".join(PROFILE_OUTPUTS)))
    pings = sum(N for N, M in sizes); samples = sum(N * M for N, M in sizes)
    stats = np.zeros(max(pings, 1), PING_DTYPE) if "stats" in want else None
    diff = np.zeros(max(samples, 1), np.int16) if "diff" in want else None
    return stats, diff, (ProfileInfo() if "info" in want else None)


def _profile_result(sizes, stats, diff, info):
    """-> (rows of PING_DTYPE over the pings of the profiled frames, the residual layers as a list of N x M int16 arrays, ProfileInfo)"""
    layers = None
    if diff is not None:
        layers, o = [], 0
        for N, M in sizes:
            layers.append(diff[o:o + N * M].reshape(N, M)); o += N * M
    return (stats[:sum(N for N, M in sizes)] if stats is not None else None), layers, info


def canvas_params_default():
    p = CanvasParams(); lib().dsss_canvas_params_default(C.byref(p)); return p


def mosaic_footprint_steps(footprint, cell, sx, sy):
    """dsss_mosaic_footprint_steps: the sub-samples along the step (sx, sy) on a grid of edge `cell` under `footprint` (a FootprintParams
    or (max_steps, max_gap)).  Host arithmetic, no context."""
    L = lib()
    n = C.c_int32(-1)
    fp = _footprint(footprint)
    rc = L.dsss_mosaic_footprint_steps(C.byref(fp) if fp is not None else None, C.c_double(cell), C.c_double(sx), C.c_double(sy), C.byref(n))
    if rc != 0:
        raise _host_error(L, "dsss_mosaic_footprint_steps", rc)
    return int(n.value)


def _reg_pairs(pairs):
    """[(a, b), ...] -> (the pairs as an n x 2 int32 array, their a column, their b column), each contiguous"""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    return pairs, np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])


def reg_params_default():
    r = RegParams(); lib().dsss_reg_params_default(C.byref(r)); return r


def mosaic_register_peak(sums, radius, min_cells, cell):
    """dsss_mosaic_register_peak: the score, peak, tie and sub-cell rules on one pair's table of shift sums ((2 radius + 1)^2 x 6 uint64,
    dy-major; n, Sa, Sb, Sab, Saa, Sbb) -> RegResult.  Host arithmetic, no context."""
    L = lib()
    out = RegResult()
    if sums is not None:
        sums = np.ascontiguousarray(sums, np.uint64)
        if 0 <= int(radius) <= 16 and sums.size != (2 * int(radius) + 1) ** 2 * 6:
            raise ValueError("mosaic_register_peak: %d sums for radius %d" % (sums.size, radius))
    rc = L.dsss_mosaic_register_peak(_ptr(sums), int(radius), int(min_cells), C.c_double(cell), C.byref(out))
    if rc != 0:
        e = DsssError("dsss_mosaic_register_peak: %s (radius %r, min_cells %r, cell %r)" % (L.dsss_strerror(rc).decode(), radius, min_cells, cell))
        e.code = rc
        raise e
    return out


def reg_edge_params_default():
    e = RegEdgeParams(); lib().dsss_reg_edge_params_default(C.byref(e)); return e


def register_edge(seg, grid, rows_a, base_a, rows_b, base_b, params=None):
    """dsss_register_edge: one row of REGSEG_DTYPE (or a RegSeg) as a pose-graph edge.  rows_a, rows_b: the "r p y x y z" rows of the
    pair's two frames under the registered trajectory, base_a, base_b: the pose-graph index of each frame's first ping, params: a
    RegEdgeParams (None = the defaults) -> a record of LCEDGE_DTYPE, or None when the segment is rejected.  Host arithmetic, no context."""
    L = lib()
    if seg is not None and not isinstance(seg, RegSeg):
        seg = RegSeg.from_buffer_copy(np.asarray(seg, REGSEG_DTYPE).tobytes())
    if rows_a is not None:
        rows_a = np.ascontiguousarray(rows_a, np.float64).reshape(-1, 6)
    if rows_b is not None:
        rows_b = np.ascontiguousarray(rows_b, np.float64).reshape(-1, 6)
    edge = np.zeros(1, LCEDGE_DTYPE)
    rc = L.dsss_register_edge(C.byref(seg) if seg is not None else None, C.byref(grid) if grid is not None else None,
                              _ptr(rows_a), 0 if rows_a is None else len(rows_a), int(base_a), _ptr(rows_b), 0 if rows_b is None else len(rows_b),
                              int(base_b), C.byref(params) if params is not None else None, _ptr(edge))
    if rc < 0:
        e = DsssError("dsss_register_edge: %s" % L.dsss_strerror(rc).decode())
        e.code = rc
        raise e
    return edge[0] if rc == 1 else None


def reg_yaw_params_default():
    y = RegYawParams(); lib().dsss_reg_yaw_params_default(C.byref(y)); return y


def reg_edge_yaw_params_default():
    e = RegEdgeYawParams(); lib().dsss_reg_edge_yaw_params_default(C.byref(e)); return e


def _host_error(L, name, rc):
    e = DsssError("%s: %s" % (name, L.dsss_strerror(rc).decode()))
    e.code = rc
    return e


def register_rotate_rows(rows_b, p0, p1, theta):
    """dsss_register_rotate_rows: the pings [p0, p1) of the "r p y x y z" rows rows_b turned by theta (radians) about the position of ping
    (p0 + p1) // 2 -> (p1 - p0) x 6.  theta == 0 copies the rows.  Host arithmetic, no context."""
    L = lib()
    if rows_b is not None:
        rows_b = np.ascontiguousarray(rows_b, np.float64).reshape(-1, 6)
    out = np.zeros((max(int(p1) - int(p0), 1), 6), np.float64)
    rc = L.dsss_register_rotate_rows(_ptr(rows_b), 0 if rows_b is None else len(rows_b), int(p0), int(p1), C.c_double(theta), _ptr(out))
    if rc != 0:
        raise _host_error(L, "dsss_register_rotate_rows", rc)
    return out


def register_yaw_peak(per_angle, step):
    """dsss_register_yaw_peak: the angle rule on the records of one (pair, segment) under the nyaw = len(per_angle) angles of a fan
    (REG_DTYPE rows) -> (k, yaw_on_border, theta, theta_hat).  Host arithmetic, no context."""
    L = lib()
    per_angle = np.ascontiguousarray(per_angle, REG_DTYPE)
    k = C.c_int32(0); border = C.c_int32(0); theta = C.c_double(0.0); hat = C.c_double(0.0)
    rc = L.dsss_register_yaw_peak(_ptr(per_angle), len(per_angle), C.c_double(step), C.byref(k), C.byref(border), C.byref(theta), C.byref(hat))
    if rc != 0:
        raise _host_error(L, "dsss_register_yaw_peak", rc)
    return k.value, border.value, theta.value, hat.value


def register_edge_yaw(seg, grid, rows_a, base_a, rows_b, base_b, params=None):
    """dsss_register_edge_yaw: register_edge for one row of REGSEGYAW_DTYPE (or a RegSegYaw); params: a RegEdgeYawParams that names the
    fan the row was registered with (None = the defaults, a fan of one angle) -> a record of LCEDGE_DTYPE, or None when the row is rejected."""
    L = lib()
    if seg is not None and not isinstance(seg, RegSegYaw):
        seg = RegSegYaw.from_buffer_copy(np.asarray(seg, REGSEGYAW_DTYPE).tobytes())
    if rows_a is not None:
        rows_a = np.ascontiguousarray(rows_a, np.float64).reshape(-1, 6)
    if rows_b is not None:
        rows_b = np.ascontiguousarray(rows_b, np.float64).reshape(-1, 6)
    edge = np.zeros(1, LCEDGE_DTYPE)
    rc = L.dsss_register_edge_yaw(C.byref(seg) if seg is not None else None, C.byref(grid) if grid is not None else None,
                                  _ptr(rows_a), 0 if rows_a is None else len(rows_a), int(base_a), _ptr(rows_b), 0 if rows_b is None else len(rows_b),
                                  int(base_b), C.byref(params) if params is not None else None, _ptr(edge))
    if rc < 0:
        raise _host_error(L, "dsss_register_edge_yaw", rc)
    return edge[0] if rc == 1 else None


def reg_pyr_params_default():
    q = RegPyrParams(); lib().dsss_reg_pyr_params_default(C.byref(q)); return q


def register_pyr_step(sums, radius, min_cells, cell, level, cx, cy):
    """dsss_register_pyr_step: the level rule of the cell pyramid on one table of shift sums ((2 radius + 1)^2 x 6 uint64) of level
    `level` around the centre (cx, cy); min_cells and cell are the level-0 values -> (RegResult with the centre added, usable, next):
    next = the centre (2 tx, 2 ty) of the level below, None at level 0 or without a usable shift.  Host arithmetic, no context."""
    L = lib()
    out = RegResult()
    if sums is not None:
        sums = np.ascontiguousarray(sums, np.uint64)
        if 0 <= int(radius) <= 16 and sums.size != (2 * int(radius) + 1) ** 2 * 6:
            raise ValueError("register_pyr_step: %d sums for radius %d" % (sums.size, radius))
    usable = C.c_int32(0); nx = C.c_int32(0); ny = C.c_int32(0)
    rc = L.dsss_register_pyr_step(_ptr(sums), int(radius), int(min_cells), C.c_double(cell), int(level), int(cx), int(cy), C.byref(out),
                                  C.byref(usable), C.byref(nx), C.byref(ny))
    if rc != 0:
        raise _host_error(L, "dsss_register_pyr_step", rc)
    return out, usable.value, ((nx.value, ny.value) if usable.value and int(level) > 0 else None)


class Context:
    """thin RAII wrapper over dsss_ctx"""

    def __init__(self, max_frames, device=0):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.dsss_create(int(device), int(max_frames), C.byref(h))
        if rc != 0:
            raise DsssError("dsss_create: %s" % self.L.dsss_strerror(rc).decode())
        self.h = h
        self.max_frames = max_frames

    def close(self):
        for cv in list(self.__dict__.get("_canvases", ())):      # the canvases that are left go first: dsss_destroy would free them under their wrappers
            cv.close()
        if getattr(self, "h", None):
            self.L.dsss_destroy(self.h)
            self.h = None
        for k in ("_keep", "_pinned"):      # nothing of the caller's stays referenced by a closed context
            self.__dict__.pop(k, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            e = DsssError("%s: %s (%s)" % (what, self.L.dsss_strerror(rc).decode(),
                                           self.L.dsss_last_error(self.h).decode()))
            e.code = rc
            raise e

    # ---- params
    def default_params(self):
        mp, op, mt, pg = MaskParams(), OrbParams(), MatchParams(), PGParams()
        self.L.dsss_mask_params_default(C.byref(mp)); self.L.dsss_orb_params_default(C.byref(op))
        self.L.dsss_match_params_default(C.byref(mt)); self.L.dsss_pg_params_default(C.byref(pg))
        return mp, op, mt, pg

    def set_params(self, mask=None, orb=None, match=None, pg=None):
        self._chk(self.L.dsss_set_params(self.h, C.byref(mask) if mask else None, C.byref(orb) if orb else None,
                                         C.byref(match) if match else None, C.byref(pg) if pg else None), "dsss_set_params")

    def sync(self):
        self._chk(self.L.dsss_sync(self.h), "dsss_sync")

    # ---- ranks (one process per GPU)
    def comm_unique_id(self):
        buf = np.zeros(128, np.uint8)
        rc = self.L.dsss_comm_unique_id(_ptr(buf))
        if rc != 0:
            raise DsssError("dsss_comm_unique_id: %s" % self.L.dsss_strerror(rc).decode())
        return buf

    def comm_init_rccl(self, uid128, rank, world):
        uid128 = np.ascontiguousarray(uid128, np.uint8); assert uid128.size == 128
        self._chk(self.L.dsss_comm_init(self.h, _ptr(uid128), int(rank), int(world)), "dsss_comm_init")

    def comm_init_callback(self, rank, world, fn):
        """fn(op, array): op 0 = sum the float64 array over the ranks in place, op 1 = all-gather: array is (world, n) uint8
        with this rank's row filled in"""
        def _cb(user, op, buf, n):
            try:
                if op == 0:
                    fn(0, np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_double)), shape=(n,)))
                else:
                    fn(1, np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint8)), shape=(world, n)))
                return 0
            except Exception as ex:                      # never let an exception cross the C boundary
                import traceback; traceback.print_exc()
                return 1
        self._cb_keep = COMM_FN(_cb)
        self._chk(self.L.dsss_comm_init_callback(self.h, int(rank), int(world), self._cb_keep, None), "dsss_comm_init_callback")

    def comm_init_device_callback(self, rank, world, fn):
        """fn(op, dev_ptr, n, stream): the library's collectives handed over as DEVICE buffers (dsss_comm_init_device_callback); op 0:
        n doubles to be summed in place, op 1: world x n bytes with this rank's slice in place; work must be ordered on `stream`"""
        def _cb(user, op, buf, n, stream):
            try:
                fn(int(op), int(buf or 0), int(n), int(stream or 0))
                return 0
            except Exception:
                import traceback; traceback.print_exc()
                return 1
        self._dcb_keep = COMM_DEV_FN(_cb)
        self._chk(self.L.dsss_comm_init_device_callback(self.h, int(rank), int(world), self._dcb_keep, None), "dsss_comm_init_device_callback")

    def comm_destroy(self):
        self._chk(self.L.dsss_comm_destroy(self.h), "dsss_comm_destroy")

    def comm_stats(self):
        r = C.c_int(); w = C.c_int(); b = C.c_double(); n = C.c_int64()
        self._chk(self.L.dsss_comm_stats(self.h, C.byref(r), C.byref(w), C.byref(b), C.byref(n)), "dsss_comm_stats")
        return r.value, w.value, b.value, n.value

    def frame_owner(self, nframes, frame):
        return self.L.dsss_comm_frame_owner(self.h, int(nframes), int(frame))

    def features_allgather(self, nframes):
        self._chk(self.L.dsss_features_allgather(self.h, int(nframes)), "dsss_features_allgather")

    def set_pg_partitions(self, nparts):
        self._chk(self.L.dsss_set_pg_partitions(self.h, int(nparts)), "dsss_set_pg_partitions")

    # ---- frames
    def frame_set(self, fid, raw, N, M, pose6, alt, gr, raw_type=None):
        """dsss_frame_set_typed.  raw: None, a numpy array or a torch tensor (host or device) of uint8, uint16, float32 or float64, taken as
        it is; raw_type only for a tensor whose dtype cannot say it (raw_type_of)."""
        pose6 = np.ascontiguousarray(pose6, np.float64); alt = np.ascontiguousarray(alt, np.float64)
        gr = np.ascontiguousarray(gr, np.float64)
        assert pose6.shape == (N, 6) and alt.shape == (N,) and gr.shape == (M // 2,)
        rt = RAW_F64 if raw is None else raw_type_of(raw, raw_type)
        if isinstance(raw, np.ndarray):
            raw = np.ascontiguousarray(raw); assert raw.shape == (N, M)
        self._keep = getattr(self, "_keep", {}); self._keep[fid] = raw      # keep device tensors alive
        self._chk(self.L.dsss_frame_set_typed(self.h, fid, _ptr(raw), rt, N, M, _ptr(pose6), _ptr(alt), _ptr(gr)), "dsss_frame_set_typed")

    def frames_args(self, ids, raws, Ns, Ms, poses, alts, grs, raw_types=None):
        """The ARGUMENT ARRAYS of dsss_frames_set_typed (ids, types, sizes, four arrays of per-frame pointers) built and validated once:
        what a C++ caller of the C ABI simply holds.  Geometry arrays must be float64 and C-contiguous; raws may hold None, host arrays
        or CUDA tensors (contiguous; uint8, uint16, float32 or float64, each frame its own: raw_type_of).  The object keeps every array
        alive; frames_set(args) is then the bare C call."""
        return FramesArgs(ids, raws, Ns, Ms, poses, alts, grs, raw_types)

    def frames_set(self, ids, raws=None, Ns=None, Ms=None, poses=None, alts=None, grs=None, raw_types=None):
        """dsss_frames_set_typed: one call for many frames.  Either the seven per-frame lists, or one FramesArgs built by frames_args()."""
        a = ids if isinstance(ids, FramesArgs) else FramesArgs(ids, raws, Ns, Ms, poses, alts, grs, raw_types)
        self._keep = getattr(self, "_keep", {})
        self._keep.update(a.keep)                              # the library borrows device images until the frame is set again
        self._chk(self.L.dsss_frames_set_typed(self.h, a.n, _ptr(a.ids), _ptr(a.p_raw), _ptr(a.raw_type), _ptr(a.N), _ptr(a.M), _ptr(a.p_pose), _ptr(a.p_alt), _ptr(a.p_gr)), "dsss_frames_set_typed")

    def frame_raw_info(self, fid):
        """dsss_frame_raw_info: (raw_type, where, owned_bytes); where: 0 none, 1 borrowed device pointer, 2 owned device copy, 3 owned copy
        whose upload from a page-locked host image is still pending."""
        t = C.c_int(0); w = C.c_int(0); b = C.c_size_t(0)
        self._chk(self.L.dsss_frame_raw_info(self.h, int(fid), C.byref(t), C.byref(w), C.byref(b)), "dsss_frame_raw_info")
        return t.value, w.value, b.value

    def frame_raw_stats(self, fid):
        """dsss_frame_raw_stats: (mean, min) of the raw image as the extraction computes them."""
        out = np.zeros(2, np.float64)
        self._chk(self.L.dsss_frame_raw_stats(self.h, int(fid), _ptr(out)), "dsss_frame_raw_stats")
        return float(out[0]), float(out[1])

    def extract(self, fid):
        n = C.c_int(0)
        self._chk(self.L.dsss_extract(self.h, fid, C.byref(n)), "dsss_extract")
        return n.value

    def extract_many(self, ids):
        ids = np.ascontiguousarray(ids, np.int32)
        self._chk(self.L.dsss_extract_many(self.h, _ptr(ids), len(ids)), "dsss_extract_many")

    def frame_norm(self, fid, N, M):
        norm = np.zeros((N, M), np.uint8); mask = np.zeros((N, M), np.uint8)
        self._chk(self.L.dsss_frame_get_norm(self.h, fid, _ptr(norm), _ptr(mask)), "dsss_frame_get_norm")
        return norm, mask

    def frame_level(self, fid, level, cap_rows, cap_cols):
        img = np.zeros(cap_rows * cap_cols, np.uint8); r = C.c_int(0); c = C.c_int(0)
        self._chk(self.L.dsss_frame_get_level(self.h, fid, level, _ptr(img), C.byref(r), C.byref(c)), "dsss_frame_get_level")
        return img[:r.value * c.value].reshape(r.value, c.value).copy()

    def frame_candidates(self, fid, level, cap=200000):
        x = np.zeros(cap, np.float32); y = np.zeros(cap, np.float32); r = np.zeros(cap, np.float32); n = C.c_int(0)
        self._chk(self.L.dsss_frame_get_candidates(self.h, fid, level, _ptr(x), _ptr(y), _ptr(r), cap, C.byref(n)), "dsss_frame_get_candidates")
        return x[:n.value].copy(), y[:n.value].copy(), r[:n.value].copy()

    def features_get(self, fid, cap=16384):
        kps = np.zeros(cap, KP_DTYPE); desc = np.zeros((cap, 32), np.uint8); geo = np.zeros((cap, 2), np.float64)
        n = C.c_int(0)
        self._chk(self.L.dsss_features_get(self.h, fid, _ptr(kps), _ptr(desc), _ptr(geo), cap, C.byref(n)), "dsss_features_get")
        return kps[:n.value].copy(), desc[:n.value].copy(), geo[:n.value].copy()

    def features_get_sift(self, fid, cap=16384):
        """Frame::dst of the SIFT call site: n x 128 float32 (integer-valued 0..255)"""
        d = np.zeros((cap, 128), np.float32); n = C.c_int(0)
        self._chk(self.L.dsss_features_get_sift(self.h, fid, _ptr(d), cap, C.byref(n)), "dsss_features_get_sift")
        return d[:n.value].copy()

    def features_set_sift(self, fid, d128):
        d = np.ascontiguousarray(d128, np.float32).reshape(-1, 128)
        self._chk(self.L.dsss_features_set_sift(self.h, fid, _ptr(d), len(d)), "dsss_features_set_sift")

    def features_set(self, fid, N, M, kps, desc, geo=None, bbox=None):
        kps = np.ascontiguousarray(kps, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        if geo is not None: geo = np.ascontiguousarray(geo, np.float64).reshape(-1, 2)
        if bbox is not None: bbox = np.ascontiguousarray(bbox, np.float64)
        self._chk(self.L.dsss_features_set(self.h, fid, N, M, _ptr(kps), _ptr(desc), _ptr(geo), _ptr(bbox), len(kps)), "dsss_features_set")

    def frame_bbox(self, fid):
        bb = np.zeros(4, np.float64)
        self._chk(self.L.dsss_frame_bbox(self.h, fid, _ptr(bb)), "dsss_frame_bbox")
        return bb

    def frame_geo(self, fid, N, M):
        """Frame::geo_img in full (dsss_frame_get_geo): two N x M float64 arrays (x, y)"""
        gx = np.empty((N, M), np.float64); gy = np.empty((N, M), np.float64)
        self._chk(self.L.dsss_frame_get_geo(self.h, fid, _ptr(gx), _ptr(gy)), "dsss_frame_get_geo")
        return gx, gy

    def overlap(self, a, b):
        v = C.c_float(0)
        self._chk(self.L.dsss_overlap(self.h, a, b, C.byref(v)), "dsss_overlap")
        return v.value

    def pack_bytes(self):
        return int(self.L.dsss_features_pack_bytes(self.h))

    def features_pack(self, fid, buf):
        """dsss_features_pack: the frame's record [int32 n, N, M, 0][bbox 4 f64][kps K][desc K x 32][geo K x 2 f64]( + [desc128 K x 128]
        under DESC_SIFT128) written into buf: pack_bytes() bytes of a contiguous uint8 numpy array, of a torch tensor on the host or
        on the device, or at a raw address.  Only the first n rows of a section mean anything.  DESC_SIFT128 on a frame without SIFT
        rows: DSSS_E_STATE, and buf is not written."""
        self._chk(self.L.dsss_features_pack(self.h, fid, _ptr(buf)), "dsss_features_pack")

    def features_unpack(self, fid, buf):
        """dsss_features_unpack: a record of features_pack's layout (numpy array, host or device tensor, raw address) into frame fid.
        A count outside [0, K]: DSSS_E_CAPACITY; another N x M than the geometry the frame has: DSSS_E_ARG; the frame stays as it was."""
        self._chk(self.L.dsss_features_unpack(self.h, fid, _ptr(buf)), "dsss_features_unpack")

    # ---- matcher
    def match_pairs(self, src, tgt):
        src = np.ascontiguousarray(src, np.int32); tgt = np.ascontiguousarray(tgt, np.int32)
        self._chk(self.L.dsss_match_pairs(self.h, _ptr(src), _ptr(tgt), len(src)), "dsss_match_pairs")

    def match_dir(self, pair, d, cap=16384):
        nn = np.zeros(cap, np.int32); co = np.zeros(cap, np.int32)
        hist = C.c_int(0); cnt = C.c_int(0); model = C.c_double(0)
        self._chk(self.L.dsss_match_get_dir(self.h, pair, d, _ptr(nn), _ptr(co), cap, C.byref(hist), C.byref(cnt), C.byref(model)), "dsss_match_get_dir")
        return nn, co, hist.value, cnt.value, model.value

    def pair_is_active(self, pair):
        """False for a pair whose geo bounding boxes are disjoint (provably no match; skipped before any kernel runs)"""
        a = C.c_int(0)
        self._chk(self.L.dsss_match_pair_active(self.h, int(pair), C.byref(a)), "dsss_match_pair_active")
        return bool(a.value)

    def match_rows(self, pair):
        n = C.c_int(0)
        self._chk(self.L.dsss_match_get_rows(self.h, pair, None, 0, C.byref(n)), "dsss_match_get_rows")
        rows = np.zeros((max(n.value, 1), 6), np.float64)
        self._chk(self.L.dsss_match_get_rows(self.h, pair, _ptr(rows), len(rows), C.byref(n)), "dsss_match_get_rows")
        return rows[:n.value].copy()

    def match_kp7(self, pair):
        n = C.c_int(0)
        self._chk(self.L.dsss_match_get_kp7(self.h, pair, None, 0, C.byref(n)), "dsss_match_get_kp7")
        out = np.zeros((max(n.value, 1), 7), np.float64)
        self._chk(self.L.dsss_match_get_kp7(self.h, pair, _ptr(out), len(out), C.byref(n)), "dsss_match_get_kp7")
        return out[:n.value].copy()

    def match_total(self):
        a = C.c_int(0); b = C.c_int(0)
        self._chk(self.L.dsss_match_total(self.h, C.byref(a), C.byref(b)), "dsss_match_total")
        return a.value, b.value

    def descriptor_distance(self, fa, ia, fb, ib):
        d = C.c_int(0)
        self._chk(self.L.dsss_descriptor_distance(self.h, fa, ia, fb, ib, C.byref(d)), "dsss_descriptor_distance")
        return d.value

    # ---- optimizer
    def lc_solve_all(self):
        self._chk(self.L.dsss_lc_solve_all(self.h), "dsss_lc_solve_all")

    def lc_get(self, pair):
        n = C.c_int(0)
        self._chk(self.L.dsss_lc_get(self.h, pair, None, 0, C.byref(n)), "dsss_lc_get")
        out = np.zeros(max(n.value, 1), LC_DTYPE)
        self._chk(self.L.dsss_lc_get(self.h, pair, _ptr(out), len(out), C.byref(n)), "dsss_lc_get")
        return out[:n.value].copy()

    def lc_solve(self, id_s, id_t, kp7):
        kp7 = np.ascontiguousarray(kp7, np.float64).reshape(-1, 7)
        out = np.zeros(max(len(kp7), 1), LC_DTYPE)
        self._chk(self.L.dsss_lc_solve(self.h, id_s, id_t, _ptr(kp7), len(kp7), _ptr(out)), "dsss_lc_solve")
        return out[:len(kp7)].copy()

    def lc_solve_pairs(self, src, tgt, kp7_list):
        """LoopClosingTFs of many pairs in one launch from caller-built kp7 lists (dsss_lc_solve_pairs)"""
        src = np.ascontiguousarray(src, np.int32); tgt = np.ascontiguousarray(tgt, np.int32)
        off = np.zeros(len(src) + 1, np.int32)
        for p, k in enumerate(kp7_list):
            off[p + 1] = off[p] + len(k)
        kp7 = np.ascontiguousarray(np.concatenate([np.asarray(k, np.float64).reshape(-1, 7) for k in kp7_list]) if len(kp7_list) else np.zeros((0, 7)))
        self._chk(self.L.dsss_lc_solve_pairs(self.h, _ptr(src), _ptr(tgt), len(src), _ptr(kp7) if len(kp7) else None, _ptr(off)), "dsss_lc_solve_pairs")

    def triangulate(self, id_s, id_t, kp7):
        kp7 = np.ascontiguousarray(kp7, np.float64).reshape(-1, 7)
        out = np.zeros((max(len(kp7), 1), 7))
        self._chk(self.L.dsss_triangulate(self.h, id_s, id_t, _ptr(kp7), len(kp7), _ptr(out)), "dsss_triangulate")
        return out[:len(kp7)].copy()

    def triangulate_poses(self, kp7, in27):
        kp7 = np.ascontiguousarray(kp7, np.float64).reshape(-1, 7); in27 = np.ascontiguousarray(in27, np.float64).reshape(-1, 27)
        out = np.zeros((max(len(kp7), 1), 7))
        self._chk(self.L.dsss_triangulate_poses(self.h, _ptr(kp7), _ptr(in27), len(kp7), _ptr(out)), "dsss_triangulate_poses")
        return out[:len(kp7)].copy()

    def posegraph_select(self, nframes, cap=1 << 20):
        edges = np.zeros(cap, LCEDGE_DTYPE); n = C.c_int(0)
        self._chk(self.L.dsss_posegraph_select(self.h, nframes, _ptr(edges), cap, C.byref(n)), "dsss_posegraph_select")
        return edges[:n.value].copy()

    def _pinned_f64(self, key, shape):
        """page-locked output buffer (device-to-host copies into it run at PCIe speed), reused by the next call with
        the same key and shape: copy the result if it has to outlive the next solve"""
        cache = self.__dict__.setdefault("_pinned", {})
        buf = cache.get((key, shape))
        if buf is None:
            try:
                import torch
                buf = torch.empty(shape, dtype=torch.float64, pin_memory=True).numpy()
            except Exception:
                buf = np.empty(shape, np.float64)
            cache[(key, shape)] = buf
        return buf

    def posegraph_solve(self, nframes, total, want_rpy=True, pinned=False):
        """poses: total x 12 (R row-major, t); rpy: the reference's trajectory rows (roll pitch yaw x y z) or None.
        pinned=True returns views of page-locked buffers owned by this Context (overwritten by its next solve)."""
        poses = self._pinned_f64("poses", (total, 12)) if pinned else np.empty((total, 12), np.float64)
        stats = np.zeros(4, np.float64)
        rpy = np.empty((total, 6), np.float64) if want_rpy else None
        self._chk(self.L.dsss_posegraph_solve(self.h, nframes, _ptr(poses), _ptr(rpy) if want_rpy else None, _ptr(stats)), "dsss_posegraph_solve")
        return poses, rpy, stats

    def posegraph_update(self, nframes, total, want_rpy=False):
        """online use (dsss_posegraph_update): frames 0..nframes-1, started from the previous update's estimate, on the accumulated
        loop closures; consumes the LC result set the context holds.  Returns poses (total x 12), rpy or None, stats."""
        poses = np.empty((total, 12), np.float64); stats = np.zeros(4, np.float64)
        rpy = np.empty((total, 6), np.float64) if want_rpy else None
        self._chk(self.L.dsss_posegraph_update(self.h, nframes, _ptr(poses), _ptr(rpy) if want_rpy else None, _ptr(stats)), "dsss_posegraph_update")
        return poses, rpy, stats

    def posegraph_update_window(self, nframes, total, window, want_poses=True):
        """the incremental form (dsss_posegraph_update_window): only the last `window` frames are solved, conditioned on the frozen estimate
        of everything before them.  Returns (poses of ALL pings or None, stats of the window's LM)."""
        poses = np.empty((total, 12), np.float64) if want_poses else None
        stats = np.zeros(4, np.float64)
        self._chk(self.L.dsss_posegraph_update_window(self.h, nframes, int(window), _ptr(poses) if want_poses else None, None, _ptr(stats)), "dsss_posegraph_update_window")
        return poses, stats

    def posegraph_reset(self):
        self._chk(self.L.dsss_posegraph_reset(self.h), "dsss_posegraph_reset")

    def posegraph_online_edges(self):
        return int(self.L.dsss_posegraph_online_edges(self.h))

    def posegraph_solve_edges(self, dr6, edges):
        dr6 = np.ascontiguousarray(dr6, np.float64).reshape(-1, 6)
        edges = np.ascontiguousarray(edges, LCEDGE_DTYPE)
        poses = np.zeros((len(dr6), 12), np.float64); stats = np.zeros(4, np.float64)
        self._chk(self.L.dsss_posegraph_solve_edges(self.h, _ptr(dr6), len(dr6), _ptr(edges), len(edges), _ptr(poses), _ptr(stats)),
                  "dsss_posegraph_solve_edges")
        return poses, stats

    def posegraph_edge_report(self, dr6, edges, poses12):
        """dsss_posegraph_edge_report: every factor of the graph (dr6 chain + edges) evaluated at poses12 (total x 12; a numpy array or a
        torch tensor, host or device) -> (chi2[ne], r6[ne, 6] whitened residuals, sums3 = 0.5 sum r^2 of the chain, of the loop closures,
        and their sum, the LM objective)"""
        dr6 = np.ascontiguousarray(dr6, np.float64).reshape(-1, 6)
        edges = np.ascontiguousarray(edges, LCEDGE_DTYPE)
        if isinstance(poses12, np.ndarray) or not hasattr(poses12, "data_ptr"):
            poses12 = np.ascontiguousarray(poses12, np.float64).reshape(-1, 12)
        if len(poses12) != len(dr6) or (hasattr(poses12, "data_ptr") and (str(poses12.dtype) != "torch.float64" or poses12.numel() != len(dr6) * 12)):
            raise ValueError("posegraph_edge_report: poses12 must be %d x 12 float64" % len(dr6))
        ne = len(edges)
        chi2 = np.zeros(ne, np.float64); r6 = np.zeros((ne, 6), np.float64); sums = np.zeros(3, np.float64)
        self._chk(self.L.dsss_posegraph_edge_report(self.h, _ptr(dr6), len(dr6), _ptr(edges), ne, _ptr(poses12), _ptr(chi2), _ptr(r6), _ptr(sums)),
                  "dsss_posegraph_edge_report")
        return chi2, r6, sums

    def gate_params_default(self):
        g = PGGateParams(); self.L.dsss_pg_gate_params_default(C.byref(g)); return g

    def posegraph_solve_gated(self, dr6, edges, gate=None):
        """dsss_posegraph_solve_gated: solve, drop the worst decade of the closures whose chi2 exceeds the gate, solve again (gate: a
        PGGateParams, None = the defaults) -> (poses, stats of the last solve, keep[ne] bool, chi2[ne] of ALL edges at the result, solves)"""
        dr6 = np.ascontiguousarray(dr6, np.float64).reshape(-1, 6)
        edges = np.ascontiguousarray(edges, LCEDGE_DTYPE)
        ne = len(edges)
        poses = np.zeros((len(dr6), 12), np.float64); stats = np.zeros(4, np.float64)
        keep = np.zeros(ne, np.uint8); chi2 = np.zeros(ne, np.float64); ns = C.c_int(0)
        self._chk(self.L.dsss_posegraph_solve_gated(self.h, _ptr(dr6), len(dr6), _ptr(edges), ne, C.byref(gate) if gate is not None else None,
                                                    _ptr(poses), _ptr(stats), _ptr(keep), _ptr(chi2), C.byref(ns)), "dsss_posegraph_solve_gated")
        return poses, stats, keep.astype(bool), chi2, ns.value

    def posegraph_schedule(self):
        """panel levels of the last solve: (levels[n][4] = items, widest panel columns, tallest rows below, interface flag; trials)"""
        n = C.c_int(0); t = C.c_int(0)
        self._chk(self.L.dsss_posegraph_schedule_get(self.h, None, 0, C.byref(n), C.byref(t)), "dsss_posegraph_schedule_get")
        lv = np.zeros((max(n.value, 1), 4), np.int32)
        self._chk(self.L.dsss_posegraph_schedule_get(self.h, _ptr(lv), n.value, C.byref(n), C.byref(t)), "dsss_posegraph_schedule_get")
        return lv[:n.value], t.value

    # ---- mosaic
    @staticmethod
    def _mosaic_traj(ids, rpy6, ping_off):
        ids = np.ascontiguousarray(ids, np.int32)
        if rpy6 is not None:
            rpy6 = np.ascontiguousarray(rpy6, np.float64); assert rpy6.ndim == 2 and rpy6.shape[1] == 6
        if ping_off is not None:
            ping_off = np.ascontiguousarray(ping_off, np.int32); assert ping_off.shape == ids.shape
        return ids, rpy6, ping_off

    def mosaic_bounds(self, ids, rpy6=None, ping_off=None):
        """union of the frames' geo extremes under the trajectory (rpy6 rows "r p y x y z", frame ids[i] from row ping_off[i]; None: the
        dead-reckoning poses the frames were set with) -> (xmin, xmax, ymin, ymax)"""
        ids, rpy6, ping_off = self._mosaic_traj(ids, rpy6, ping_off)
        bb = np.zeros(4, np.float64)
        self._chk(self.L.dsss_mosaic_bounds(self.h, _ptr(ids), len(ids), _ptr(rpy6), _ptr(ping_off), _ptr(bb)), "dsss_mosaic_bounds")
        return bb

    def mosaic_render(self, ids, params, rpy6=None, ping_off=None, download=True):
        """the frames' normalised images binned into the grid `params` -> (sum, cnt, img): H x W uint32, uint32, uint8.
        download=False renders on the device only and returns None (timing)."""
        ids, rpy6, ping_off = self._mosaic_traj(ids, rpy6, ping_off)
        out = (np.empty((params.H, params.W), np.uint32), np.empty((params.H, params.W), np.uint32),
               np.empty((params.H, params.W), np.uint8)) if download else (None, None, None)
        self._chk(self.L.dsss_mosaic_render(self.h, _ptr(ids), len(ids), _ptr(rpy6), _ptr(ping_off), C.byref(params),
                                            _ptr(out[0]), _ptr(out[1]), _ptr(out[2])), "dsss_mosaic_render")
        return out if download else None

    def mosaic_consistency(self, ids, params, rpy6=None, ping_off=None):
        """what overlapping frames say about a cell -> (nfr, s1, s2, score): frames that see the cell, sum and sum of squares of their
        mean grey levels (H x W uint32), and the pooled standard deviation over the cells seen by two frames or more"""
        ids, rpy6, ping_off = self._mosaic_traj(ids, rpy6, ping_off)
        nfr, s1, s2 = (np.empty((params.H, params.W), np.uint32) for _ in range(3))
        score = C.c_double(0.0)
        self._chk(self.L.dsss_mosaic_consistency(self.h, _ptr(ids), len(ids), _ptr(rpy6), _ptr(ping_off), C.byref(params),
                                                 _ptr(nfr), _ptr(s1), _ptr(s2), C.byref(score)), "dsss_mosaic_consistency")
        return nfr, s1, s2, score.value

    def mosaic_composite(self, ids, params, mode=COMP_NEAR, fill_radius=0, rpy6=None, ping_off=None, want=("img", "src_frame", "src_ping", "src_col", "fill")):
        """dsss_mosaic_composite: one winning sample per cell under the priority `mode` (a COMP_* value or its name), enclosed holes
        filled within fill_radius cells -> (layers, info): layers = a dict of the H x W layers named in `want` (img uint8; src_frame,
        src_ping, src_col int32, -1 where empty; fill uint8), info = a CompInfo or None.  want=() builds the mosaic on the device and
        downloads nothing (timing); add "info" to get the cell counts alone."""
        ids, rpy6, ping_off = self._mosaic_traj(ids, rpy6, ping_off)
        known = [n for n, _ in COMP_LAYERS] + ["info"]
        for w in want:
            if w not in known:
                raise ValueError("mosaic_composite: no layer %r (%s)" % (w, ", ".join(known)))
        out = {n: np.empty((params.H, params.W), t) for n, t in COMP_LAYERS if n in want}
        info = CompInfo() if (out or "info" in want) else None
        cp = CompParams(int(COMP_MODES.get(mode, mode)), int(fill_radius))
        self._chk(self.L.dsss_mosaic_composite(self.h, _ptr(ids), len(ids), _ptr(rpy6), _ptr(ping_off), C.byref(params), C.byref(cp),
                                               *[_ptr(out.get(n)) for n, _ in COMP_LAYERS], C.byref(info) if info is not None else None), "dsss_mosaic_composite")
        return out, info

    def mosaic_render_footprint(self, ids, params, rpy6=None, ping_off=None, download=True, footprint=None):
        """dsss_mosaic_render_footprint: mosaic_render over the sub-samples of the samples' footprints.  footprint: a FootprintParams or
        (max_steps, max_gap), None = the library's defaults (4, 1.0); max_steps 1 gives mosaic_render's layers bit for bit."""
        ids, rpy6, ping_off = self._mosaic_traj(ids, rpy6, ping_off)
        fp = _footprint(footprint)
        out = (np.empty((params.H, params.W), np.uint32), np.empty((params.H, params.W), np.uint32),
               np.empty((params.H, params.W), np.uint8)) if download else (None, None, None)
        self._chk(self.L.dsss_mosaic_render_footprint(self.h, _ptr(ids), len(ids), _ptr(rpy6), _ptr(ping_off), C.byref(params),
                                                      C.byref(fp) if fp is not None else None, _ptr(out[0]), _ptr(out[1]), _ptr(out[2])),
                  "dsss_mosaic_render_footprint")
        return out if download else None

    def mosaic_composite_footprint(self, ids, params, mode=COMP_NEAR, fill_radius=0, rpy6=None, ping_off=None,
                                   want=("img", "src_frame", "src_ping", "src_col", "fill"), footprint=None):
        """dsss_mosaic_composite_footprint: mosaic_composite over the sub-samples of the samples' footprints, each with its parent's key,
        value and source.  footprint as in mosaic_render_footprint; everything else as in mosaic_composite."""
        ids, rpy6, ping_off = self._mosaic_traj(ids, rpy6, ping_off)
        known = [n for n, _ in COMP_LAYERS] + ["info"]
        for w in want:
            if w not in known:
                raise ValueError("mosaic_composite_footprint: no layer %r (%s)" % (w, ", ".join(known)))
        out = {n: np.empty((params.H, params.W), t) for n, t in COMP_LAYERS if n in want}
        info = CompInfo() if (out or "info" in want) else None
        cp = CompParams(int(COMP_MODES.get(mode, mode)), int(fill_radius))
        fp = _footprint(footprint)
        self._chk(self.L.dsss_mosaic_composite_footprint(self.h, _ptr(ids), len(ids), _ptr(rpy6), _ptr(ping_off), C.byref(params), C.byref(cp),
                                                         C.byref(fp) if fp is not None else None, *[_ptr(out.get(n)) for n, _ in COMP_LAYERS],
                                                         C.byref(info) if info is not None else None), "dsss_mosaic_composite_footprint")
        return out, info

    def mosaic_gain_stats(self, ids, use_mask=1, bands=None):
        """dsss_mosaic_gain_stats: the column statistics of the listed frames (all of one M) -> (S, C), M uint64 each: the sum and the
        number of the kept samples of every column (use_mask != 0: the samples the filter mask keeps).  bands (a GainBands or
        (alt0, dalt, nbands)): dsss_mosaic_gain_stats_banded -> (S, C) of nbands x M, per band of the pings' altitudes."""
        ids = np.ascontiguousarray(ids, np.int32)
        M = C.c_int(0)                                           # the columns of the first frame: the library holds every other one to it
        if len(ids):
            self._chk(self.L.dsss_frame_get_level(self.h, int(ids[0]), 0, None, None, C.byref(M)), "dsss_mosaic_gain_stats (the frame's size)")
        M = M.value
        if bands is None:
            S = np.zeros(max(M, 1), np.uint64); Cn = np.zeros(max(M, 1), np.uint64)
            self._chk(self.L.dsss_mosaic_gain_stats(self.h, _ptr(ids), len(ids), int(use_mask), _ptr(S), _ptr(Cn)), "dsss_mosaic_gain_stats")
            return S[:M], Cn[:M]
        b = _bands(bands)
        nb = min(max(int(b.nbands), 1), 16)                     # room for what a valid call writes: the library refuses the rest
        S = np.zeros((nb, max(M, 1)), np.uint64); Cn = np.zeros_like(S)
        self._chk(self.L.dsss_mosaic_gain_stats_banded(self.h, _ptr(ids), len(ids), int(use_mask), C.byref(b), _ptr(S), _ptr(Cn)), "dsss_mosaic_gain_stats_banded")
        return S.reshape(-1)[:nb * M].reshape(nb, M), Cn.reshape(-1)[:nb * M].reshape(nb, M)

    def mosaic_gain_set(self, table, bands=None):
        """dsss_mosaic_gain_set: install the range-gain table (M uint16, Q8) every mosaic and registration entry applies from now on;
        None clears it.  bands (a GainBands or (alt0, dalt, nbands)): dsss_mosaic_gain_set_banded with a table of nbands x M."""
        if table is None:
            self._chk(self.L.dsss_mosaic_gain_set(self.h, None, 0), "dsss_mosaic_gain_set")
            return
        table = np.ascontiguousarray(table, np.uint16)
        if bands is None:
            self._chk(self.L.dsss_mosaic_gain_set(self.h, _ptr(table), int(table.size)), "dsss_mosaic_gain_set")
            return
        b = _bands(bands)
        if table.ndim != 2 or table.shape[0] != b.nbands:
            raise ValueError("mosaic_gain_set: a table of shape %s for %d bands" % (table.shape, b.nbands))
        self._chk(self.L.dsss_mosaic_gain_set_banded(self.h, _ptr(table), int(table.shape[1]), C.byref(b)), "dsss_mosaic_gain_set_banded")

    def mosaic_gain_get_banded(self):
        """dsss_mosaic_gain_get_banded: the table in force, whatever its bands, read back from the device -> (table nbands x M uint16,
        GainBands), or None when none is set"""
        M = C.c_int(0); b = GainBands()
        rc = self.L.dsss_mosaic_gain_get_banded(self.h, None, 0, C.byref(M), C.byref(b))      # the size first: *M and the bands are written also without room
        if M.value == 0:
            self._chk(rc, "dsss_mosaic_gain_get_banded")
            return None
        out = np.empty((b.nbands, M.value), np.uint16)
        self._chk(self.L.dsss_mosaic_gain_get_banded(self.h, _ptr(out), int(out.size), C.byref(M), C.byref(b)), "dsss_mosaic_gain_get_banded")
        return out, b

    def frame_corrected(self, id):
        """dsss_frame_get_corrected: the frame's normalised image under the range-gain table in force (N x M uint8; with no table the
        normalised image itself)"""
        N = C.c_int(0); M = C.c_int(0)
        self._chk(self.L.dsss_frame_get_level(self.h, int(id), 0, None, C.byref(N), C.byref(M)), "dsss_frame_get_corrected (the frame's size)")
        out = np.empty((max(N.value, 1), max(M.value, 1)), np.uint8)
        self._chk(self.L.dsss_frame_get_corrected(self.h, int(id), _ptr(out)), "dsss_frame_get_corrected")
        return out

    def mosaic_gain_get(self, cap=None):
        """dsss_mosaic_gain_get: the table in force, read back from the device (M uint16), or None when none is set.  cap: the room
        offered (None: what the table needs)"""
        M = C.c_int(0)
        if cap is None:                                          # ask for the size first: *M is written also when the room does not suffice
            rc = self.L.dsss_mosaic_gain_get(self.h, None, 0, C.byref(M))
            if M.value == 0:
                self._chk(rc, "dsss_mosaic_gain_get")
                return None
            cap = M.value
        out = np.empty(max(int(cap), 1), np.uint16)
        self._chk(self.L.dsss_mosaic_gain_get(self.h, _ptr(out), int(cap), C.byref(M)), "dsss_mosaic_gain_get")
        return out[:M.value].copy() if M.value else None

    def mosaic_register(self, ids, params, pairs, reg=None, rpy6=None, ping_off=None, want_sums=False):
        """dense overlap registration of the frame pairs `pairs` = [(a, b), ...] (frame ids, both in ids) under the trajectory: frame b slid
        over frame a within reg.radius cells (reg: a RegParams, None = the defaults) -> rows of REG_DTYPE, one per pair: the peak shift
        in cells, the offset in metres that b lies from where the overlap says it belongs, ZNCC and cells at the peak and at zero shift.
        want_sums=True returns (rows, sums) with sums[npairs, 2 r + 1, 2 r + 1, 6] uint64 (dy, dx; n, Sa, Sb, Sab, Saa, Sbb)."""
        ids, rpy6, ping_off = self._mosaic_traj(ids, rpy6, ping_off)
        pairs, pa, pb = _reg_pairs(pairs)
        r = reg if reg is not None else reg_params_default()
        S = 2 * max(0, min(int(r.radius), 16)) + 1
        out = np.zeros(len(pairs), REG_DTYPE)
        sums = np.zeros((len(pairs), S, S, 6), np.uint64) if want_sums else None
        self._chk(self.L.dsss_mosaic_register(self.h, _ptr(ids), len(ids), _ptr(rpy6), _ptr(ping_off), C.byref(params), _ptr(pa), _ptr(pb),
                                              len(pairs), C.byref(r), _ptr(out), _ptr(sums)), "dsss_mosaic_register")
        return (out, sums) if want_sums else out

    def mosaic_register_segments(self, ids, params, pairs, seg_pings, reg=None, rpy6=None, ping_off=None, want_sums=False, cap=None):
        """the registration of mosaic_register with frame b of every pair cut into segments of seg_pings pings, each slid over the whole
        of frame a -> rows of REGSEG_DTYPE, by pair and then by segment: the pair's index, the segment and its pings [p0, p1), the
        record r of the segment's table, and the centroid sums sx, sy of the overlapping cells at the peak.  want_sums=True returns
        (rows, sums) with sums[nseg, 2 r + 1, 2 r + 1, 6] uint64.  cap: room for that many rows (None: as many as there will be)."""
        ids, rpy6, ping_off = self._mosaic_traj(ids, rpy6, ping_off)
        pairs, pa, pb = _reg_pairs(pairs)
        r = reg if reg is not None else reg_params_default()
        S = 2 * max(0, min(int(r.radius), 16)) + 1
        args = (self.h, _ptr(ids), len(ids), _ptr(rpy6), _ptr(ping_off), C.byref(params), _ptr(pa), _ptr(pb), len(pairs), int(seg_pings), C.byref(r))
        return self._reg_segment_rows(self.L.dsss_mosaic_register_segments, "dsss_mosaic_register_segments", args, REGSEG_DTYPE, (S, S, 6), want_sums, cap)

    def _reg_segment_rows(self, fn, name, args, dtype, sums_shape, want_sums, cap):
        """the capacity protocol of the three segment entries: fn(*args, rows, cap, &nseg, sums) -> the nseg rows of `dtype`, with
        want_sums (rows, sums[nseg, *sums_shape]).  cap None: as many rows as there will be."""
        nseg = C.c_int(0)
        if cap is None:                                    # the library counts the rows before it launches anything: ask with no room
            one = np.zeros(1, dtype)
            rc = fn(*args, _ptr(one), 0, C.byref(nseg), None)
            if rc != -5:                                   # DSSS_E_CAPACITY: nseg rows are needed; 0: there are none; anything else is an error
                self._chk(rc, name)
            cap = nseg.value
        out = np.zeros(max(cap, 1), dtype)
        sums = np.zeros((max(cap, 1),) + tuple(sums_shape), np.uint64) if want_sums else None
        self._chk(fn(*args, _ptr(out), int(cap), C.byref(nseg), _ptr(sums)), name)
        out = out[:nseg.value]
        return (out, sums[:nseg.value]) if want_sums else out

    def _reg_edges(self, fn, name, dtype, pair_of, ids, params, pairs, segs, edge_params, rpy6, ping_off, cap):
        """the body of the two edges bindings: segs as rows of `dtype`, pair_of(segs) = the pair each row names -> (edges, edge_seg)"""
        ids, rpy6, ping_off = self._mosaic_traj(ids, rpy6, ping_off)
        pairs, pa, pb = _reg_pairs(pairs)
        segs = np.ascontiguousarray(segs, dtype)
        if len(segs) and (pair_of(segs).min() < 0 or pair_of(segs).max() >= len(pairs)):
            raise ValueError("%s: a row names a pair outside the %d given" % (name[len("dsss_"):], len(pairs)))
        cap = len(segs) if cap is None else int(cap)
        edges = np.zeros(max(cap, 1), LCEDGE_DTYPE); src = np.zeros(max(cap, 1), np.int32); ne = C.c_int(0)
        self._chk(fn(self.h, _ptr(ids), len(ids), _ptr(rpy6), _ptr(ping_off), C.byref(params), _ptr(pa), _ptr(pb), _ptr(segs), len(segs),
                     C.byref(edge_params) if edge_params is not None else None, _ptr(edges), _ptr(src), cap, C.byref(ne)), name)
        return edges[:ne.value].copy(), src[:ne.value].copy()

    def mosaic_register_edges(self, ids, params, pairs, segs, edge_params=None, rpy6=None, ping_off=None, cap=None):
        """register_edge on every row of segs (REGSEG_DTYPE, as mosaic_register_segments returned them for `pairs`) under the trajectory
        that was registered -> (edges, edge_seg): the accepted rows as LCEDGE_DTYPE records over the pose-graph indices ping_off[i] + ping
        (ping_off None: the frames of ids one behind the other), and the row each edge came from.  Launches no GPU work."""
        return self._reg_edges(self.L.dsss_mosaic_register_edges, "dsss_mosaic_register_edges", REGSEG_DTYPE, lambda s: s["pair"],
                               ids, params, pairs, segs, edge_params, rpy6, ping_off, cap)

    def mosaic_register_segments_yaw(self, ids, params, pairs, seg_pings, yaw=None, reg=None, rpy6=None, ping_off=None, want_sums=False, cap=None):
        """mosaic_register_segments with every segment registered under the angles of the fan `yaw` (a RegYawParams, None = the default
        of one angle) as well -> rows of REGSEGYAW_DTYPE: s = the row of the best angle k, with theta, theta_hat, yaw_on_border and the
        unrotated angle's ZNCC.  want_sums=True returns (rows, sums) with sums[nseg, nyaw, 2 r + 1, 2 r + 1, 6] uint64."""
        ids, rpy6, ping_off = self._mosaic_traj(ids, rpy6, ping_off)
        pairs, pa, pb = _reg_pairs(pairs)
        r = reg if reg is not None else reg_params_default()
        y = yaw if yaw is not None else reg_yaw_params_default()
        S = 2 * max(0, min(int(r.radius), 16)) + 1
        A = max(1, min(int(y.nyaw), 17))
        args = (self.h, _ptr(ids), len(ids), _ptr(rpy6), _ptr(ping_off), C.byref(params), _ptr(pa), _ptr(pb), len(pairs), int(seg_pings), C.byref(r),
                C.byref(y))
        return self._reg_segment_rows(self.L.dsss_mosaic_register_segments_yaw, "dsss_mosaic_register_segments_yaw", args, REGSEGYAW_DTYPE, (A, S, S, 6),
                                      want_sums, cap)

    def mosaic_register_edges_yaw(self, ids, params, pairs, segs, edge_params=None, rpy6=None, ping_off=None, cap=None):
        """mosaic_register_edges for the rows of mosaic_register_segments_yaw (REGSEGYAW_DTYPE); edge_params: a RegEdgeYawParams that names
        the fan the rows were registered with -> (edges, edge_seg).  The edges measure the heading too.  Launches no GPU work."""
        return self._reg_edges(self.L.dsss_mosaic_register_edges_yaw, "dsss_mosaic_register_edges_yaw", REGSEGYAW_DTYPE, lambda s: s["s"]["pair"],
                               ids, params, pairs, segs, edge_params, rpy6, ping_off, cap)

    def mosaic_register_segments_pyr(self, ids, params, pairs, seg_pings, pyr=None, reg=None, rpy6=None, ping_off=None, want_sums=False, cap=None):
        """mosaic_register_segments coarse to fine over the cell pyramid `pyr` (a RegPyrParams, None = the default of one level): the top
        level searches reg.radius of its cells, every level below pyr.refine cells around twice the shift found above -> rows of
        REGSEGPYR_DTYPE: s = the row of the finest level with a usable peak (accepted by mosaic_register_edges only when it finished at
        level 0 away from every border), level, border_mask and the shift and ZNCC per level.  want_sums=True returns (rows, sums)
        with sums[nseg, (2 r + 1)^2 + (levels - 1) (2 refine + 1)^2, 6] uint64: the top level's table, then those of the levels below."""
        ids, rpy6, ping_off = self._mosaic_traj(ids, rpy6, ping_off)
        pairs, pa, pb = _reg_pairs(pairs)
        r = reg if reg is not None else reg_params_default()
        q = pyr if pyr is not None else reg_pyr_params_default()
        S = 2 * max(0, min(int(r.radius), 16)) + 1
        lv = max(1, min(int(q.levels), 4)); Sr = 2 * max(0, min(int(q.refine), 16)) + 1
        args = (self.h, _ptr(ids), len(ids), _ptr(rpy6), _ptr(ping_off), C.byref(params), _ptr(pa), _ptr(pb), len(pairs), int(seg_pings), C.byref(r),
                C.byref(q))
        return self._reg_segment_rows(self.L.dsss_mosaic_register_segments_pyr, "dsss_mosaic_register_segments_pyr", args, REGSEGPYR_DTYPE,
                                      (S * S + (lv - 1) * Sr * Sr, 6), want_sums, cap)

    def mosaic_register_peaks(self, sums, radius, min_cells, cell, ntables=None, out=None):
        """dsss_mosaic_register_peaks: the peak rule on many tables at once, on the device -> rows of REG_DTYPE, row k bit for bit what
        mosaic_register_peak gives for table k.  sums: a numpy array of ntables x (2 radius + 1)^2 x 6 uint64 (ntables from its
        size), or device memory -- a torch tensor, or an address -- with ntables given.  out: a REG_DTYPE array to write into."""
        S = 2 * int(radius) + 1
        if isinstance(sums, np.ndarray):
            sums = np.ascontiguousarray(sums, np.uint64)
            if ntables is None:
                if not 0 <= int(radius) <= 16 or sums.size % (S * S * 6):
                    raise ValueError("mosaic_register_peaks: %d sums for radius %d" % (sums.size, radius))
                ntables = sums.size // (S * S * 6)
        elif ntables is None:
            raise ValueError("mosaic_register_peaks: ntables is needed with device memory")
        if out is None:
            out = np.zeros(max(int(ntables), 0), REG_DTYPE)
        assert out.dtype == REG_DTYPE and out.flags.c_contiguous and len(out) >= ntables
        self._chk(self.L.dsss_mosaic_register_peaks(self.h, _ptr(sums), int(ntables), int(radius), int(min_cells), C.c_double(cell),
                                                    _ptr(out) if len(out) else None), "dsss_mosaic_register_peaks")
        return out

    def mosaic_register_info(self):
        """dsss_mosaic_register_info -> a RegCallInfo of the last mosaic_register* call of this context that succeeded"""
        info = RegCallInfo()
        self._chk(self.L.dsss_mosaic_register_info(self.h, C.byref(info)), "dsss_mosaic_register_info")
        return info

    def _frame_sizes(self, ids):
        """(N, M) of the listed frames; (0, 0) for one the library does not know: the entry that follows refuses it"""
        out = []
        for i in ids:
            N = C.c_int(0); M = C.c_int(0)
            rc = self.L.dsss_frame_get_level(self.h, int(i), 0, None, C.byref(N), C.byref(M))
            out.append((N.value, M.value) if rc == 0 else (0, 0))
        return out

    def profile_mosaic(self, ids, params, prof=None, min_count=1, rpy6=None, ping_off=None, want=PROFILE_OUTPUTS):
        """dsss_profile_mosaic (include/dsss_profile.h): every ping of the frames ids[prof] (prof None: all, in order) held against the
        mosaic of all OTHER listed frames on the grid `params` -> (stats, diff, info): rows of PING_DTYPE, one per ping, the frames one
        after the other; the residual layers as a list of N x M int16 arrays (PROFILE_NONE where a sample is not compared); a
        ProfileInfo.  Each is None when it is not named in `want`."""
        ids, rpy6, ping_off = self._mosaic_traj(ids, rpy6, ping_off)
        pr = None if prof is None else np.ascontiguousarray(prof, np.int32)
        which = range(len(ids)) if pr is None else [int(k) for k in pr if 0 <= int(k) < len(ids)]
        sizes = self._frame_sizes([ids[k] for k in which])
        stats, diff, info = _profile_outputs(sizes, want)
        pp = ProfileParams(int(min_count), 0)
        room = pr if pr is None or len(pr) else np.zeros(1, np.int32)      # an empty list still goes down as a list
        self._chk(self.L.dsss_profile_mosaic(self.h, _ptr(ids), len(ids), _ptr(rpy6), _ptr(ping_off), C.byref(params), _ptr(room), 0 if pr is None else len(pr),
                                             C.byref(pp), _ptr(stats), _ptr(diff), C.byref(info) if info is not None else None), "dsss_profile_mosaic")
        return _profile_result(sizes, stats, diff, info)

    def canvas(self, params, footprint=None, move=CANVAS_MOVE_AUTO):
        """dsss_canvas_create: a mosaic canvas on the grid `params` (include/dsss_canvas.h).  footprint: None = point samples, a
        FootprintParams or (max_steps, max_gap) = a footprint canvas; move: CANVAS_MOVE_AUTO or CANVAS_MOVE_SPLIT"""
        return Canvas(self, params, footprint, move)

    # ---- instrumentation
    def profile(self, on=True):
        self._chk(self.L.dsss_profile_enable(self.h, 1 if on else 0), "dsss_profile_enable")

    def profile_reset(self):
        self._chk(self.L.dsss_profile_reset(self.h), "dsss_profile_reset")

    def profile_get(self):
        K = len(K_NAMES)                                   # == DSSS_K_COUNT (include/dsss.h)
        ms = np.zeros(K, np.float64); n = np.zeros(K, np.int64); wk = np.zeros(K, np.float64)
        self._chk(self.L.dsss_profile_get(self.h, _ptr(ms), _ptr(n)), "dsss_profile_get")
        self._chk(self.L.dsss_profile_get_work(self.h, _ptr(wk)), "dsss_profile_get_work")
        return {K_NAMES[i]: (float(ms[i]), int(n[i]), float(wk[i])) for i in range(K) if not K_NAMES[i].startswith("k2")}


class Canvas:
    """dsss_canvas (include/dsss_canvas.h): a mean mosaic kept on the device; frames are put (added, moved, skipped) and removed, and it
    always reads what a fresh render of its frames under their stored rows reads.  Made by Context.canvas."""

    def __init__(self, ctx, params, footprint=None, move=CANVAS_MOVE_AUTO):
        self.ctx, self.L, self.h = ctx, ctx.L, None
        cp = canvas_params_default()
        cp.move = int(move)
        if footprint is not None:
            cp.footprint = 1; cp.fp = _footprint(footprint)
        h = C.c_void_p()
        ctx._chk(self.L.dsss_canvas_create(ctx.h, C.byref(params), C.byref(cp), C.byref(h)), "dsss_canvas_create")
        self.h = h
        self.W, self.H = int(params.W), int(params.H)
        ctx.__dict__.setdefault("_canvases", []).append(self)

    def close(self):
        if self.h is not None:
            if self.ctx.h:
                self.L.dsss_canvas_destroy(self.h)
            self.h = None
            self.ctx._canvases.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def put(self, ids, rpy6=None, ping_off=None):
        """dsss_canvas_put -> a CanvasPutInfo.  rpy6 (host rows "r p y x y z", frame ids[i] from row ping_off[i]) or None: the poses the
        frames were set with"""
        ids, rpy6, ping_off = Context._mosaic_traj(ids, rpy6, ping_off)
        info = CanvasPutInfo()
        self.ctx._chk(self.L.dsss_canvas_put(self.h, _ptr(ids), len(ids), _ptr(rpy6), _ptr(ping_off), C.byref(info)), "dsss_canvas_put")
        return info

    def remove(self, ids):
        ids = np.ascontiguousarray(ids, np.int32)
        self.ctx._chk(self.L.dsss_canvas_remove(self.h, _ptr(ids), len(ids)), "dsss_canvas_remove")

    def clear(self):
        self.ctx._chk(self.L.dsss_canvas_clear(self.h), "dsss_canvas_clear")

    def read(self, win=None, want=("sum", "cnt", "img")):
        """dsss_canvas_read -> (sum, cnt, img) of the window win = (ox, oy, bw, bh), None: the grid; bh x bw uint32, uint32, uint8 (None for
        a layer not in `want`)"""
        w = None if win is None else np.ascontiguousarray(win, np.int32)
        bw, bh = (self.W, self.H) if w is None else (max(int(w[2]), 0), max(int(w[3]), 0))
        out = [np.empty((bh, bw), t) if n in want else None for n, t in (("sum", np.uint32), ("cnt", np.uint32), ("img", np.uint8))]
        self.ctx._chk(self.L.dsss_canvas_read(self.h, _ptr(w), _ptr(out[0]), _ptr(out[1]), _ptr(out[2])), "dsss_canvas_read")
        return tuple(out)

    def dirty(self, reset=True):
        """dsss_canvas_dirty -> (ox, oy, bw, bh) of everything touched since the last reset, None when nothing was"""
        w = np.zeros(4, np.int32)
        self.ctx._chk(self.L.dsss_canvas_dirty(self.h, _ptr(w), 1 if reset else 0), "dsss_canvas_dirty")
        return tuple(int(v) for v in w) if w[2] > 0 else None

    def frames(self):
        """the ids on the canvas, ascending"""
        n = C.c_int(0)
        self.L.dsss_canvas_frames(self.h, None, 0, C.byref(n))      # (DSSS_E_CAPACITY with frames on it: the call that asks how many)
        ids = np.zeros(max(n.value, 1), np.int32)
        self.ctx._chk(self.L.dsss_canvas_frames(self.h, _ptr(ids), len(ids), C.byref(n)), "dsss_canvas_frames")
        return ids[:n.value].tolist()

    def rows(self, id, N):
        """dsss_canvas_rows: the N x 6 rows frame `id` is on the canvas with, downloaded from the canvas's device copy"""
        out = np.empty((int(N), 6), np.float64)
        self.ctx._chk(self.L.dsss_canvas_rows(self.h, int(id), _ptr(out)), "dsss_canvas_rows")
        return out

    def profile(self, ids, min_count=1, want=PROFILE_OUTPUTS):
        """dsss_profile_canvas (include/dsss_profile.h): every ping of the listed frames of the canvas held against the canvas without the
        frame itself -> (stats, diff, info) as Context.profile_mosaic returns them, the frames in the order of ids.  The canvas is not
        changed."""
        ids = np.ascontiguousarray(ids, np.int32)
        sizes = self.ctx._frame_sizes(ids)
        stats, diff, info = _profile_outputs(sizes, want)
        pp = ProfileParams(int(min_count), 0)
        self.ctx._chk(self.L.dsss_profile_canvas(self.h, _ptr(ids), len(ids), C.byref(pp), _ptr(stats), _ptr(diff),
                                                 C.byref(info) if info is not None else None), "dsss_profile_canvas")
        return _profile_result(sizes, stats, diff, info)

    def frame_window(self, id, rows=None):
        """dsss_canvas_frame_window -> (ox, oy, bw, bh) of the cells frame `id` can reach under `rows` (None: the stored rows), None when
        it reaches none"""
        if rows is not None:
            rows = np.ascontiguousarray(rows, np.float64)
        w = np.zeros(4, np.int32)
        self.ctx._chk(self.L.dsss_canvas_frame_window(self.h, int(id), _ptr(rows), _ptr(w)), "dsss_canvas_frame_window")
        return tuple(int(v) for v in w) if w[2] > 0 else None
