"""ctypes binding of include/tokenhmr_hip.h (libtokenhmr_hip.so).

There is NO CPU fallback: if the shared library is missing or a symbol is absent this module
raises, so a GPU box can never silently run anything but the HIP path.

The header is the one source of every signature: bind() types each entry point from its prototype there (param_ctype is the rule).
Hand-written here are only the struct mirrors and the constants, and tests/test_cabi_header.py holds both against the header.
"""
import ctypes as C
import functools
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtokenhmr_hip.so")
# the EXPERIMENTS build of the same sources (-DTHMR_EXPERIMENTS: THMR_* environment knobs, debug hooks, kernels that lost their A/B —
# csrc/common.h).  Never the product path: tests and scripts ask for it with load(exp=True) / Engine(..., experiments=True), or a whole
# process with THMR_LIB=exp.
LIB_PATH_EXP = os.path.join(_HERE, "lib", "libtokenhmr_hip_exp.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "tokenhmr_hip.h")

ABI_VERSION = 5
# thmr_config.flags (header: THMR_CFG_*)
CFG_VIT_GEMM_F32, CFG_NO_PERSISTENT, CFG_HEAD_HMR2 = 1, 2, 8
PROF_NAMES = ["gemm_qkv", "gemm_proj", "gemm_fc1", "gemm_fc2", "attention", "layernorm", "patch_embed",
              "dec_kv", "head", "lbs"]


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("vit_depth", C.c_int32), ("dec_depth", C.c_int32),
                ("max_batch", C.c_int32), ("device", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


class TensorDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("numel", C.c_int64),
                ("on_device", C.c_int32), ("reserved", C.c_int32)]


class SmplDesc(C.Structure):
    _fields_ = [("v_template", C.c_void_p), ("shapedirs", C.c_void_p), ("posedirs", C.c_void_p),
                ("J_regressor", C.c_void_p), ("lbs_weights", C.c_void_p), ("J19_regressor", C.c_void_p),
                ("parents", C.c_void_p), ("extra_verts", C.c_void_p), ("joint_map", C.c_void_p),
                ("on_device", C.c_int32), ("update_hips", C.c_int32)]


class SmplhDesc(C.Structure):
    _fields_ = [("v_template", C.c_void_p), ("shapedirs", C.c_void_p), ("posedirs", C.c_void_p), ("J_regressor", C.c_void_p),
                ("lbs_weights", C.c_void_p), ("parents", C.c_void_p), ("extra_verts", C.c_void_p), ("on_device", C.c_int32),
                ("reserved", C.c_int32)]


MEAN_ROW_DIST_WS = 256      # header: THMR_MEAN_ROW_DIST_WS
# thmr_val_loss / thmr_op_token_ce (header: THMR_VAL_LOSS_*, THMR_TOKEN_CE_WS_PER_ROW): modes and workspace floats per item / per row
VAL_LOSS_PLAIN, VAL_LOSS_LOOSE = 0, 1
VAL_LOSS_WS_PER_ITEM, TOKEN_CE_WS_PER_ROW = 5, 1
# thmr_val_loss_grad (header: THMR_LOSS_GRAD_*): the slots of its host table of device pointers
LOSS_GRAD_KP2D, LOSS_GRAD_KP3D, LOSS_GRAD_JOINTS, LOSS_GRAD_CAM, LOSS_GRAD_ROTMAT, LOSS_GRAD_BETAS, LOSS_GRAD_SLOTS = 0, 1, 2, 3, 4, 5, 6
# thmr_disc_forward / thmr_disc_backward (header: THMR_DISC_*): the slots of their host table of device pointers, and the sizes
DISC_OUT, DISC_LOSS, DISC_GRAD_POSES, DISC_GRAD_BETAS, DISC_WORKSPACE, DISC_SLOTS = 0, 1, 2, 3, 4, 5
DISC_MAX_BATCH, DISC_KPAD, DISC_WEIGHT_FLOATS, DISC_WS_PER_ITEM = 256, 768, 3644480, 5665
VAL_LOSS_IN_FIELDS = ["pred_keypoints_2d", "pred_keypoints_3d", "pred_rotmat", "pred_betas", "gt_keypoints_2d", "gt_keypoints_3d", "gt_pose",
                      "gt_betas", "has_global_orient", "has_body_pose", "has_betas", "valid_3d", "kp2d_thresh", "angle_thresh"]
VAL_LOSS_OUT_FIELDS = ["losses", "per_item", "kp2d_err", "angle_err", "valid2d", "weak2d", "valid_rot", "weak_rot", "conf2d_used",
                       "conf3d_used", "has_betas_used", "running"]


class ValLossDesc(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("w_keypoints_2d", "w_keypoints_3d", "w_global_orient", "w_body_pose", "w_betas", "loose_weight")] + \
               [(n, C.c_int32) for n in ("pelvis_id", "mode", "gt_pose_is_rotmat", "reserved")]


class ValLossIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in VAL_LOSS_IN_FIELDS]


class ValLossOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in VAL_LOSS_OUT_FIELDS]


OUTPUT_FIELDS = ["pred_cam", "rotmat", "betas", "cls_logits_softmax", "pred_cam_t", "focal_length",
                 "pred_keypoints_3d", "pred_vertices", "pred_keypoints_2d", "token_idx",
                 "vit_features", "token_out", "cls_logits", "pose6d"]


class Outputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in OUTPUT_FIELDS]


class CropDesc(C.Structure):
    _fields_ = [("M", C.c_double * 6), ("sigma", C.c_double), ("truncate", C.c_double)]


class FrameCrop(C.Structure):
    """thmr_frame_crop: one item of thmr_cropper_run_frames."""
    _fields_ = [("win_dev", C.c_void_p), ("row_stride", C.c_int64), ("H", C.c_int32), ("W", C.c_int32), ("win_x0", C.c_int32),
                ("win_y0", C.c_int32), ("win_w", C.c_int32), ("win_h", C.c_int32), ("M", C.c_double * 6), ("sigma", C.c_double),
                ("truncate", C.c_double)]


class JpegInfo(C.Structure):
    """thmr_jpeg_info."""
    _fields_ = [(n, C.c_int32) for n in ("height", "width", "components", "h_samp", "v_samp", "restart_interval", "supported", "reserved")]


class JpegPlan(C.Structure):
    """thmr_jpeg_plan: what thmr_jpeg_entropy_decode kept."""
    _fields_ = [(n, C.c_int32) for n in ("height", "width", "components", "h_samp", "v_samp", "win_x0", "win_y0", "win_w", "win_h", "mcu_row0",
                                         "mcu_rows_kept", "mcu_rows_decoded")] + \
               [(n, C.c_int32 * 3) for n in ("bx0", "by0", "bw", "bh", "coef_block")] + [("n_blocks", C.c_int32), ("quant", (C.c_uint16 * 64) * 3)]


class PngItem(C.Structure):
    """thmr_png_item: one image of thmr_png_encode_batch / thmr_png_encode_host."""
    _fields_ = [("pixels", C.c_void_p), ("dtype", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32),
                ("stride_y", C.c_int64), ("stride_x", C.c_int64), ("stride_c", C.c_int64), ("scale", C.c_float), ("rounding", C.c_int32),
                ("swap_rb", C.c_int32), ("compression", C.c_int32), ("out", C.c_void_p), ("capacity", C.c_int64), ("written", C.c_int64)]


PNG_U8, PNG_F32, PNG_U16 = 0, 1, 2                  # header: THMR_PNG_*
PNG_ROUND_NEAREST, PNG_ROUND_TRUNC = 0, 1           # header: THMR_PNG_ROUND_*
PNG_FIXED, PNG_DYNAMIC = 0, 1                       # header: THMR_PNG_FIXED / _DYNAMIC
JPEG_444, JPEG_422, JPEG_420 = 0, 1, 2              # header: THMR_JPEG_* (thmr_jpeg_encode_*; 4:2:2 is refused by name)
JPEG_OPTIMIZE = 1                                   # header: THMR_JPEG_OPTIMIZE, the flag bit of thmr_jpeg_encode_*_flags


class JpegItem(C.Structure):
    """thmr_jpeg_item: one item of thmr_jpeg_decode_batch."""
    _fields_ = [("coef", C.c_void_p), ("plan", C.POINTER(JpegPlan)), ("win_x0", C.c_int32), ("win_y0", C.c_int32), ("win_w", C.c_int32),
                ("win_h", C.c_int32), ("out_dev", C.c_void_p), ("row_stride", C.c_int64)]


# thmr_png_probe / thmr_png_inflate_window: the info and the plan are int32 words (header: THMR_PNG_INFO_* / THMR_PNG_PLAN_*)
PNG_INFO_WORDS, PNG_PLAN_WORDS, PNG_PLAN_PALETTE = 8, 206, 14
PNG_INFO_FIELDS = ["height", "width", "bit_depth", "colour_type", "interlace", "bpp", "supported"]
PNG_PLAN_FIELDS = ["height", "width", "bit_depth", "colour_type", "bpp", "win_x0", "win_y0", "win_w", "win_h", "row0", "rows_kept",
                   "kept_row_bytes", "rows_inflated", "palette_entries"]


ERR_INVALID, ERR_HIP, ERR_STATE, ERR_NOMEM, ERR_UNSUPPORTED = -1, -2, -3, -4, -5      # header: thmr_status

RENDER_MAX_LIGHTS = 16
# thmr_render_desc.mode / thmr_render_light.type (header: THMR_RENDER_* / THMR_LIGHT_*)
RENDER_PER_IMAGE, RENDER_ONE_IMAGE = 0, 1
LIGHT_DIRECTIONAL, LIGHT_POINT = 0, 1


class RenderLight(C.Structure):
    _fields_ = [("type", C.c_int32), ("vec", C.c_float * 3), ("color", C.c_float * 3), ("intensity", C.c_float)]


class RenderDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("znear", C.c_float), ("samples", C.c_int32), ("mode", C.c_int32), ("translate_first", C.c_int32),
                ("rot", C.c_float * 9), ("base_color", C.c_float * 3), ("mesh_colors", C.POINTER(C.c_float)), ("bg_color", C.c_float * 3),
                ("metallic", C.c_float), ("roughness", C.c_float), ("ambient", C.c_float * 3), ("n_lights", C.c_int32),
                ("lights", RenderLight * RENDER_MAX_LIGHTS), ("out_channels", C.c_int32), ("img_mean", C.c_float * 3),
                ("img_std", C.c_float * 3), ("ids_dev", C.c_void_p)]


# thmr_sheet_desc.panels, and the draw-list records of thmr_renderer_sheet (header: THMR_SHEET_*)
SHEET_IMAGE, SHEET_FRONT, SHEET_SIDE = 1, 2, 4
SHEET_KEYPOINTS, SHEET_RECORDS, SHEET_RECORD_WORDS = 44, 49, 12


class SheetDesc(C.Structure):
    _fields_ = [("n", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("img_res", C.c_int32), ("panels", C.c_int32),
                ("nrow", C.c_int32), ("padding", C.c_int32), ("canvas_width", C.c_int32), ("canvas_height", C.c_int32)]


class GemmChoice(C.Structure):
    _fields_ = [("kind", C.c_int32), ("ksplit", C.c_int32)]


# thmr_gemm_choice.kind / thmr_vit_plan_desc.path / .attn (header: THMR_GEMM_*, THMR_VIT_PATH_*, THMR_ATTN_*)
GEMM_KINDS = ["f32_tile", "f32_tile_splitk", "f32_ring", "f32_ring16", "s3_tile", "s3_tile_splitk", "s3_stream_wide", "s3_stream_narrow",
              "s3_splitk_stream", "s3_ring"]
VIT_PATHS = ["f32", "split3", "split3_small"]
ATTN_KINDS = ["f32", "f32_keysplit", "f32_split3_out", "b16"]


class VitPlanDesc(C.Structure):
    _fields_ = [("path", C.c_int32)] + [(n, GemmChoice) for n in ("patch", "qkv", "proj", "fc1", "fc2", "to_kv")] + \
               [("attn", C.c_int32), ("bs_blk", C.c_int32), ("part2_in_scratch", C.c_int32), ("tile_opts", C.c_int32)]


class TokenizerOut(C.Structure):
    _fields_ = [("idx", C.c_void_p), ("latent", C.c_void_p), ("pose6d", C.c_void_p), ("rotmat", C.c_void_p), ("aa", C.c_void_p),
                ("commit_loss", C.c_void_p), ("perplexity", C.c_void_p), ("code_count", C.c_void_p), ("accumulate_counts", C.c_int32),
                ("reserved", C.c_int32)]


class ProfEntry(C.Structure):
    _fields_ = [("ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double), ("launches", C.c_int64)]


# every struct the header defines -> its mirror above (tests/test_cabi_header.py holds each against the compiler's layout of the header)
STRUCTS = {"thmr_config": Config, "thmr_tensor_desc": TensorDesc, "thmr_smpl_desc": SmplDesc, "thmr_smplh_desc": SmplhDesc,
           "thmr_val_loss_desc": ValLossDesc, "thmr_val_loss_in": ValLossIn, "thmr_val_loss_out": ValLossOut, "thmr_outputs": Outputs,
           "thmr_crop_desc": CropDesc, "thmr_frame_crop": FrameCrop, "thmr_jpeg_info": JpegInfo, "thmr_jpeg_plan": JpegPlan,
           "thmr_jpeg_item": JpegItem, "thmr_png_item": PngItem, "thmr_render_light": RenderLight, "thmr_render_desc": RenderDesc,
           "thmr_sheet_desc": SheetDesc, "thmr_gemm_choice": GemmChoice, "thmr_vit_plan_desc": VitPlanDesc,
           "thmr_tokenizer_out": TokenizerOut, "thmr_prof_entry": ProfEntry}

_RESTYPES = {"int": C.c_int, "int64_t": C.c_int64, "void": None, "const char*": C.c_char_p}
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_HOST_OUT = {"size_t": C.c_size_t, "int64_t": C.c_int64, "uint64_t": C.c_uint64}     # T* of these: host out-parameters, never device memory
_ADDRESSES = ("void", "float", "int32_t", "uint8_t", "int16_t")                      # T* of these, and of an opaque handle: a plain address


def parse_prototypes(text):
    """({name: (return type as written, [parameter type without `const`, blanks and the parameter's name, ...])} of every function that
    the C text declares, the set of its opaque handle types `typedef struct thmr_x thmr_x;`)."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    funcs = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t*]*?)\b(thmr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        funcs[name] = (ret.strip(), [] if params.strip() == "void" else [re.sub(r"\bconst\b|\w+\s*$|\s", "", p) for p in params.split(",")])
    return funcs, set(re.findall(r"typedef\s+struct\s+(thmr_\w+)\s+\1\s*;", text))


def param_ctype(t, opaque=()):
    """The ctypes type of one parameter type of parse_prototypes: the ONE rule every entry point is typed by.  Anything else raises."""
    base, stars = t.rstrip("*"), len(t) - len(t.rstrip("*"))
    address = base in _ADDRESSES or base in opaque
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and base in STRUCTS:
        return C.POINTER(STRUCTS[base])
    if stars == 2 and (base == "char" or address):
        return C.POINTER(C.c_char_p if base == "char" else C.c_void_p)
    if stars == 1 and base in _HOST_OUT:
        return C.POINTER(_HOST_OUT[base])
    if stars == 1 and address:
        return C.c_void_p
    raise RuntimeError(f"tokenhmr_hip.h has a parameter of type '{t}': _cabi.param_ctype() knows the scalars {sorted(_SCALARS)}, pointers "
                       f"to the structs of _cabi.STRUCTS, to {sorted(_HOST_OUT)}, to {sorted(_ADDRESSES)} and to opaque handles, and T**")


@functools.lru_cache(maxsize=None)
def _header():
    """(parse_prototypes' functions, {name: (restype, argtypes)} in ctypes) of include/tokenhmr_hip.h, read once per process."""
    with open(HEADER) as f:
        funcs, opaque = parse_prototypes(f.read())
    for name, (ret, _) in funcs.items():                 # every return type as the header writes it
        if ret not in _RESTYPES:
            raise RuntimeError(f"tokenhmr_hip.h declares {name} as returning '{ret}': _cabi knows {sorted(_RESTYPES)}")
    return funcs, {name: (_RESTYPES[ret], [param_ctype(t, opaque) for t in params]) for name, (ret, params) in funcs.items()}


def declared_functions():
    """{name: (return type, [parameter types])} of every function the header declares, as parse_prototypes gives them."""
    return dict(_header()[0])


def declared_return_types():
    """{name: return type as written}: 'int', 'int64_t', 'void' or 'const char*'."""
    return {name: ret for name, (ret, _) in _header()[0].items()}


def declared_symbols():
    """Every function the header declares (used by the symbol-export test)."""
    return sorted(_header()[0])


def bind(lib, partial=False):
    """Sets restype and argtypes, derived from the header, on every declared function that `lib` exports.  A declared function it does not
    export raises here, by name — unless `partial`: then it is left unbound and fails (AttributeError) where it is called."""
    missing = []
    for name, (restype, argtypes) in _header()[1].items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        else:
            missing.append(name)
    if missing and not partial:
        raise RuntimeError(f"libtokenhmr_hip.so lacks symbols declared in tokenhmr_hip.h: {sorted(missing)}")
    return lib


_libs = {}


def load(exp=None):
    """The shipped library, or (exp=True, or exp=None with THMR_LIB=exp in the environment) the experiments build.
    exp = a PATH (str): that very file — another BUILD of this library, e.g. the previous round's, loaded beside the current one by
    scripts/ab_same_box.py so that two builds are timed interleaved in one process on one box (A/B tooling only; ABI 3 and 4 builds
    accepted: no struct layout or signature changed between 3 and 5 — 4 changed the creation default of the ViT GEMM mode, 5 gave
    thmr_config.reserved[0] a meaning and added thmr_mode_bytes, which such a build simply lacks).  A build loaded by path is bound
    with partial=True: whatever declared function it lacks fails at the call, not here; the two builds of this tree must export all."""
    if exp is None:
        exp = os.environ.get("THMR_LIB", "") == "exp"
    if isinstance(exp, str):
        path = os.path.abspath(exp)
        exp = path
    else:
        exp = bool(exp)
        path = LIB_PATH_EXP if exp else LIB_PATH
    if exp in _libs:
        return _libs[exp]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: the HIP extension is not built. Run `python __graft_entry__.py` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
    # ONE HIP runtime per process.  libtokenhmr_hip.so needs "libamdhip64.so.7" (resolved to /opt/rocm when nothing of that soname
    # is loaded yet); PyTorch's libraries need "libamdhip64.so" and find the copy bundled under torch/lib, which the loader does NOT
    # recognise as the same library when /opt/rocm's is already mapped under the other name — two runtimes, and the second one to
    # touch the device fails (seen as "hipSetDevice failed" in thmr_create when this module was loaded before `import torch`).
    # With torch imported first its runtime carries the soname libamdhip64.so.7 and is reused here.  Hosts without PyTorch
    # (the plain C ABI) are unaffected.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    bind(lib, partial=isinstance(exp, str))
    version = lib.thmr_abi_version()
    if version != ABI_VERSION and not (isinstance(exp, str) and version in (3, 4)):    # a previous round's build, loaded by path
        raise RuntimeError("libtokenhmr_hip.so ABI version mismatch")
    _libs[exp] = lib
    return lib


class EngineError(RuntimeError):
    pass


def check(rc, engine=None, lib=None):
    if rc != 0:
        lib = lib if lib is not None else load()
        msg = lib.thmr_last_error(engine)
        raise EngineError(f"tokenhmr_hip error {rc}: {msg.decode() if msg else '?'}")


def raise_error(rc, what, msg, error=EngineError, by_code=None):
    """The one text of a failed C call: '<entry point> error <rc>: <the C message>'; by_code picks another class for some codes."""
    raise (by_code or {}).get(rc, error)(f"{what} error {rc}: {msg.decode() if msg else '?'}")


class Handle:
    """Owner of one C handle of the family `stem` (thmr_cropper -> thmr_cropper_create / _destroy / _last_error): resolves the device
    ('cuda' without an index means the CURRENT device, like Engine, not device 0), creates the handle with _open, raises the family's
    exception with the C side's own message from _check, and destroys the handle once — by close() or when the object is collected.
    last_error: the symbol that reads the message where the family has no thmr_X_last_error of its own (the body models report
    through thmr_last_error(NULL): their handles keep no string)."""
    error, error_by_code, no_gpu_error = EngineError, None, RuntimeError

    @classmethod
    def cuda_device(cls, device, needs_gpu, resolve):
        """torch.device(device), refused with `needs_gpu` unless it is a GPU.  resolve: 'cuda' without an index becomes the current
        device, which needs a GPU."""
        import torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise cls.no_gpu_error(needs_gpu)
        return torch.device("cuda", torch.cuda.current_device()) if resolve and dev.index is None else dev

    def __init__(self, device, stem, needs_gpu, last_error=None):
        self.device = self.cuda_device(device, needs_gpu, resolve=False)
        self._needs_gpu = needs_gpu
        self.lib = load()
        self._stem, self._per_handle = stem, last_error is None
        self._last_error = getattr(self.lib, last_error or stem + "_last_error")
        self.h = None

    def _index(self):
        """The device index; 'cuda' without one becomes the current device here, which needs a GPU."""
        self.device = self.cuda_device(self.device, self._needs_gpu, resolve=True)
        return self.device.index

    def _open(self, *args):
        """thmr_X_create(*args, &handle)."""
        h = C.c_void_p()
        self._check(getattr(self.lib, self._stem + "_create")(*args, C.byref(h)), self._stem + "_create")
        self.h = h

    def _check(self, rc, what):
        if rc != 0:
            raise_error(rc, what, self._last_error(self.h if self._per_handle else None), self.error, self.error_by_code)

    def close(self):
        if getattr(self, "h", None):
            getattr(self.lib, self._stem + "_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
