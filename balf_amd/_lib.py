"""ctypes binding of libbalf_hip.so (include/balf_hip.h).

There is no CPU fallback anywhere in ``balf_amd``: if the shared library is missing or the
device is not an MI355X, the calls below raise.  The library is built in-tree by
``balf_amd/csrc/build.sh`` (plain ``hipcc --offload-arch=gfx950``, see ``__graft_entry__.build``).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BALF_HIP_LIB", os.path.join(_HERE, "libbalf_hip.so"))   # override: tuning builds only

OK = 0
PREC_FP32, PREC_FP16 = 0, 1
MAX_NMS_SIZE, MAX_TOPK = 32, 16384
PYR_SRC_U8, PYR_SRC_F32, PYR_SRC_LEVEL = 0, 1, 2                   # include/balf_hip.h: balf_pyramid_level
PYR_MAX_RADIUS, MAX_PYRAMID_LEVELS = 8, 32
VAL_LEG_GREEDY, VAL_LEG_WINDOW = 0, 1                              # include/balf_hip.h: balf_val_points
NMS_MAP_GREEDY, NMS_MAP_BOX, NMS_MAP_MAX_RADIUS = 0, 1, 16         # include/balf_hip.h: balf_nms_score_map
STATUS_SCORE, STATUS_RANGE, STATUS_SE, STATUS_WORDS = 0, 1, 2, 4      # include/balf_hip.h: balf_forward_status
UNIT_RCAB, UNIT_GMLP, UNIT_POOL = 0, 1, 2                          # include/balf_hip.h: balf_train_unit_sizes
OPTIM_MAX_TENSORS = 64                                             # include/balf_hip.h: balf_adam_step / balf_sgd_step

# name -> (restype, argtypes); kept in step with include/balf_hip.h (tests/test_abi.py checks)
_vp, _i, _sz, _fp = C.c_void_p, C.c_int, C.c_size_t, C.c_void_p
PROTOTYPES = {
    "balf_abi_version": (_i, []),
    "balf_error_string": (C.c_char_p, [_i]),
    "balf_device_check": (_i, []),
    "balf_build_flags": (C.c_char_p, []),
    "balf_num_state_tensors": (_i, []),
    "balf_state_tensor_name": (C.c_char_p, [_i]),
    "balf_state_tensor_numel": (_sz, [_i]),
    "balf_packed_weights_bytes": (_sz, [_i]),
    "balf_pack_weights": (_i, [C.POINTER(_vp), _i, _i, _vp, _sz]),
    "balf_forward_workspace_bytes": (_sz, [_i, _i, _i]),
    "balf_forward_micro_batch": (_i, [_i, _i, _i]),
    "balf_forward": (_i, [_vp, _i, _fp, _i, _i, _i, _fp, _fp, _vp, _sz, _vp]),
    "balf_forward_u8": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _fp, _fp, _vp, _sz, _vp]),
    "balf_forward_status": (_i, [_vp, _i, _fp, _i, _i, _i, _fp, _fp, _vp, _sz, _vp, _vp]),
    "balf_forward_u8_status": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _fp, _fp, _vp, _sz, _vp, _vp]),
    "balf_forward_stage_view_numel": (_sz, [_i, _i, _i, _i]),
    "balf_forward_stage_view": (_i, [_i, _vp, _sz, _i, _i, _i, _i, _fp, _vp]),
    "balf_window_nms": (_i, [_fp, _i, _i, _i, _i, _i, _fp, _vp]),
    "balf_nms_topk_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "balf_nms_topk": (_i, [_fp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _fp, _vp, _vp, _sz, _vp]),
    "balf_nms_threshold": (_i, [_fp, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.c_float, _i, _vp, _fp, _vp, _vp, _sz, _vp]),
    "balf_pyramid_level": (_i, [_vp, _i, _i, _i, _i, _i, C.c_double, _i, _i, _fp, _vp]),
    "balf_nms_topk_budget": (_i, [_fp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _fp, _vp, _vp, _sz, _vp]),
    "balf_multiscale_merge": (_i, [_vp, _fp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "balf_greedy_nms_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "balf_greedy_nms": (_i, [_fp, _i, _i, _i, _i, _i, _i, _i, _i, C.c_float, _i, _i, _i, _vp, _fp, _fp, _vp, _vp, _vp,
                            _sz, _vp]),
    "balf_nms_score_map_sizes": (_i, [_i, _i, _i, _i, C.POINTER(_sz)]),
    "balf_nms_score_map": (_i, [_fp, _i, _i, _i, _i, C.c_float, _i, C.POINTER(C.c_uint64), _i, _i, _fp, _vp, _vp, _sz, _vp]),
    "balf_hardnet_num_state_tensors": (_i, []),
    "balf_hardnet_state_tensor_name": (C.c_char_p, [_i]),
    "balf_hardnet_state_tensor_numel": (_sz, [_i]),
    "balf_hardnet_packed_weights_bytes": (_sz, []),
    "balf_hardnet_pack_weights": (_i, [C.POINTER(_vp), _i, _vp, _sz]),
    "balf_hardnet_workspace_bytes": (_sz, [_i]),
    "balf_hardnet_forward": (_i, [_vp, _fp, _i, _fp, _vp, _sz, _vp]),
    "balf_hardnet_forward_masked": (_i, [_vp, _fp, _i, _i, _vp, _fp, _vp, _sz, _vp]),
    "balf_hardnet_forward_ex": (_i, [_vp, _fp, _i, _i, _vp, _i, _fp, _vp, _sz, _vp]),
    "balf_extract_patches_workspace_bytes": (_sz, [_i, _i, C.c_float]),
    "balf_extract_patches": (_i, [_vp, _i, _i, _fp, _i, C.c_float, _fp, _vp, _sz, _vp]),
    "balf_extract_patches_batch_workspace_bytes": (_sz, [_i, _i, _i, C.c_float]),
    "balf_extract_patches_batch": (_i, [_vp, _i, _i, _i, _fp, _vp, _i, C.c_float, _fp, _vp, _sz, _vp]),
    "balf_rgb_to_gray": (_i, [_vp, C.c_long, _vp, _vp]),
    "balf_match_smnn_workspace_bytes": (_sz, [_i, _i]),
    "balf_match_smnn": (_i, [_fp, _i, _fp, _i, C.c_float, _vp, _fp, _vp, _vp, _sz, _vp]),
    "balf_match_smnn_batch_workspace_bytes": (_sz, [_i, _i, _i]),
    "balf_match_smnn_batch": (_i, [_fp, _i, _vp, _fp, _i, _vp, _i, C.c_float, _vp, _fp, _vp, _vp, _sz, _vp]),
    "balf_repeatability_workspace_bytes": (_sz, [_i, _i, _i]),
    "balf_repeatability": (_i, [_vp, _i, _vp, _i, C.c_double, C.c_double, C.c_double, C.c_double, _i, _vp, _vp, _vp, _vp,
                               _vp, _sz, _vp]),
    "balf_apply_homography": (_i, [_vp, _i, _vp, _vp, _vp]),
    "balf_common_region_masks": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "balf_common_points_batch": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "balf_repeatability_batch_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "balf_repeatability_batch": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, C.c_double, C.c_double, C.c_double,
                                     C.c_double, _i, _vp, _vp, _vp, _sz, _vp]),
    "balf_common_points_index_batch": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "balf_match_accuracy_batch": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, C.POINTER(C.c_double), _i, _vp, _vp, _vp]),
    "balf_val_points_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i, _i]),
    "balf_val_points": (_i, [_fp, _i, _i, _fp, _i, _i, _i, _vp, _i, C.c_float, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "balf_resize_repeatability_batch_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "balf_resize_repeatability_batch": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, C.c_double,
                                            _vp, _vp, _vp, _sz, _vp]),
    "balf_resize_crop_u8": (_i, [_vp, _sz, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "balf_synth_pairs_workspace_bytes": (_sz, [_i, _i]),
    "balf_synth_pairs": (_i, [_vp, _sz, _vp, _vp, _i, _vp, _vp, _vp, _fp, _i, _vp, _i, _i, _fp, _fp, _fp, _fp, _vp, _vp, _sz,
                             _vp]),
    "balf_photometric_u8": (_i, [_vp, _sz, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    "balf_synth_train_pairs": (_i, [_vp, _sz, _vp, _vp, _i, _vp, _vp, _vp, _fp, _i, _vp, _i, _i, _fp, _fp, _fp, _fp, _vp, _vp, _sz,
                                   _vp, _vp, _vp]),
    "balf_detector_loss_workspace_bytes": (_sz, [_i, _i, _i]),
    "balf_detector_loss": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _fp, _fp, _vp, _fp, _vp, _sz, _vp]),
    "balf_head_train_workspace_bytes": (_sz, [C.c_long]),
    "balf_head_train_saved_bytes": (_sz, [C.c_long]),
    "balf_head_train_forward": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, C.c_double, _i, _fp, _fp, _fp, _fp, _fp,
                                    C.c_double, _vp, _vp, _sz, _vp]),
    "balf_head_train_backward": (_i, [_fp, _fp, _fp, _fp, _fp, _vp, _i, _i, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "balf_rcab_train_workspace_bytes": (_sz, [_i, _i, _i]),
    "balf_rcab_train_saved_bytes": (_sz, [_i, _i, _i]),
    "balf_rcab_train_forward": (_i, [_fp] * 12 + [_i, _i, _i, _fp, _vp, _vp, _sz, _vp]),
    "balf_rcab_train_backward": (_i, [_fp] * 7 + [_vp, _i, _i, _i] + [_fp] * 11 + [_vp, _sz, _vp]),
    "balf_rcab_train_forward_c": (_i, [_fp] * 12 + [_i, _i, _i, _i, _fp, _vp, _vp, _sz, _vp]),
    "balf_rcab_train_backward_c": (_i, [_fp] * 7 + [_vp, _i, _i, _i, _i] + [_fp] * 11 + [_vp, _sz, _vp]),
    "balf_forward_rcab_inputs": (_i, [_i, _vp, _sz, _i, _i, _i, _fp, _fp, _fp, _fp, _vp]),
    "balf_gmlp_train_workspace_bytes": (_sz, [_i, _i, _i]),
    "balf_gmlp_train_saved_bytes": (_sz, [_i, _i, _i]),
    "balf_gmlp_train_forward": (_i, [_fp, C.POINTER(_vp), _i, _i, _i, _fp, _vp, _vp, _sz, _vp]),
    "balf_gmlp_train_backward": (_i, [_fp, _fp, C.POINTER(_vp), _vp, _i, _i, _i, C.POINTER(_vp), _fp, _vp, _sz, _vp]),
    "balf_gmlp_train_forward_c": (_i, [_fp, C.POINTER(_vp), _i, _i, _i, _i, _fp, _vp, _vp, _sz, _vp]),
    "balf_gmlp_train_backward_c": (_i, [_fp, _fp, C.POINTER(_vp), _vp, _i, _i, _i, _i, C.POINTER(_vp), _fp, _vp, _sz, _vp]),
    "balf_forward_gmlp_input": (_i, [_i, _vp, _sz, _i, _i, _i, _fp, _fp, _fp, _fp, _vp]),
    "balf_linrelu_train_workspace_bytes": (_sz, [_i, _i]),
    "balf_linrelu_train_forward": (_i, [_fp, _fp, _fp, _i, _i, _fp, _vp]),
    "balf_linrelu_train_backward": (_i, [_fp, _fp, _fp, _fp, _i, _i, _fp, _fp, _fp, _vp, _sz, _vp]),
    "balf_pool_train_forward": (_i, [_fp, _i, _i, _i, _i, _fp, _vp, _vp]),
    "balf_pool_train_backward": (_i, [_fp, _vp, _i, _i, _i, _i, _fp, _vp]),
    "balf_train_unit_sizes": (_i, [_i, _i, _i, _i, _i, C.POINTER(_sz), C.POINTER(_sz)]),
    "balf_optim_chunk_elems": (_i, []),
    "balf_adam_step": (_i, [_i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int64), C.c_double,
                           C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64, _vp]),
    "balf_sgd_step": (_i, [_i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int64), C.c_double, _vp]),
    "balf_profile_num_slots": (_i, []),
    "balf_profile_slot_name": (C.c_char_p, [_i]),
    "balf_profile_begin": (_i, []),
    "balf_profile_end": (_i, [_vp, _vp]),
}


class BalfHipError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Load the library once; fail loudly when it is absent (never fall back to a CPU path)."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise BalfHipError(
                f"{LIB_PATH} not found: build it with balf_amd/csrc/build.sh (or __graft_entry__.build()); "
                "balf_amd has no CPU fallback")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(l, name)          # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        if l.balf_abi_version() != 1:
            raise BalfHipError("libbalf_hip.so ABI version mismatch")
        flags = l.balf_build_flags().decode()
        if not flags.startswith("release"):
            # a timing-ablation / instrumented build (csrc/diag.h) computes wrong results: only ever loaded on purpose
            if "BALF_HIP_LIB" not in os.environ:
                raise BalfHipError(f"{LIB_PATH} is a diagnostic build ({flags}): rebuild it with balf_amd/csrc/build.sh")
            import warnings
            warnings.warn(f"balf_amd: {LIB_PATH} is a DIAGNOSTIC build ({flags}); its results are not valid", RuntimeWarning)
        _lib = l
    return _lib


_checked_devices = set()


def require_mi355x(device) -> None:
    """Raise unless ``device`` is a gfx950 GPU (balf_device_check: the kernels are built for MI355X only).  Checked
    once per device, by every op wrapper before its first launch there."""
    import torch
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx in _checked_devices:
        return
    with torch.cuda.device(idx):
        rc = lib().balf_device_check()
    if rc != OK:
        raise BalfHipError(f"cuda:{idx} is not an MI355X (gfx950): {lib().balf_error_string(rc).decode()} ({rc})")
    _checked_devices.add(idx)


def check(rc: int, what: str) -> None:
    if rc != OK:
        raise BalfHipError(f"{what} failed: {lib().balf_error_string(rc).decode()} ({rc})")


def require_gpu_tensor(t, name: str) -> None:
    if not t.is_cuda:
        raise BalfHipError(f"{name} must live on the GPU: balf_amd has no CPU path (got device {t.device})")
    if not t.is_contiguous():
        raise BalfHipError(f"{name} must be contiguous")
    require_mi355x(t.device)


def current_stream_ptr(device) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream


# ---- the one door into the library ---------------------------------------------------------------------------
def raw_stream(index: int) -> int:
    """The current stream of device ``index`` as the pointer the library takes: torch's direct accessor where this build has
    it (a tenth of the cost of making a ``torch.cuda.Stream`` object, which shows in a 37 us step), else through that object."""
    import torch
    get = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    return get(index) if get is not None else torch.cuda.current_stream(index).cuda_stream


def on_device(dev, call):
    """The low layer: ``call(stream)`` with ``dev`` (a ``torch.device`` or a device index) current and ``stream`` its current
    stream -> what ``call`` returns.  Without the context manager when the device already is current (the common case).  For
    a caller that keeps its C arguments across calls, as the optimiser step does; everything else goes through launch()."""
    import torch
    index = dev if isinstance(dev, int) else dev.index
    current = torch.cuda.current_device()
    if index is None or index == current:
        return call(raw_stream(current))
    with torch.cuda.device(index):
        return call(raw_stream(index))


class Workspace:
    """Marks a scratch tensor among launch()'s arguments: the library takes it as two, its pointer and its byte count."""
    __slots__ = ("tensor",)

    def __init__(self, tensor):
        self.tensor = tensor


def launch(name: str, dev, *args, what=None) -> None:
    """The high layer: entry ``name`` of the library on the current stream of ``dev``, with ``dev`` current (on_device).  Of
    ``args``, a tensor goes as its ``data_ptr()``, None as NULL, a :class:`Workspace` as pointer and byte count; everything
    else -- numbers, ctypes arrays, host pointers -- goes as it is, and the stream is appended last.  A failure is reported
    under ``what or name`` (check).  The tensors are arguments of this call, so they live until the work is enqueued."""
    import torch
    fn = getattr(lib(), name, None)
    if fn is None:
        raise BalfHipError(f"{name} is not an entry of libbalf_hip.so")
    c_args = []
    for a in args:
        if isinstance(a, torch.Tensor):
            c_args.append(a.data_ptr())
        elif isinstance(a, Workspace):
            c_args += (a.tensor.data_ptr(), a.tensor.nbytes)
        else:
            c_args.append(a)
    check(on_device(dev, lambda stream: fn(*c_args, stream)), what or name)


def tensor_key(t):
    """(storage address, version) of a parameter/buffer, for the packed-weight caches.  Inference tensors
    (a model moved under torch.inference_mode()) do not track versions and cannot be modified in place."""
    try:
        return (t.data_ptr(), t._version)
    except RuntimeError:
        return (t.data_ptr(), -1)


def pack_state_dict(sd, n, name_of, numel_of, nbytes, pack, what):
    """The ``n`` tensors of ``sd`` that the library names (``name_of(i)``, ``numel_of(i)`` elements each), as contiguous fp32
    on the host, through ``pack(pointers, n, out, nbytes)`` -> the packed blob, ``nbytes`` of uint8 on the host."""
    import torch
    host = []
    for i in range(n):
        name = name_of(i).decode()
        t = sd[name].detach().to("cpu", torch.float32).contiguous()
        if t.numel() != numel_of(i):
            raise BalfHipError(f"{name}: {t.numel()} elements, library expects {numel_of(i)}")
        host.append(t)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in host])
    blob = torch.empty(nbytes, dtype=torch.uint8)
    check(pack(ptrs, n, blob.data_ptr(), nbytes), what)
    return blob
