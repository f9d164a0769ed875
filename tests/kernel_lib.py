"""ctypes binding of the sdpk_* test entries (include/sdp_kernels.h) for the per-kernel GPU tests.

Kept out of sdp/_lib.py on purpose: the package binds the stable sdp_* ABI only.  Tensors cross as NHWC CUDA tensors
(float32, or bfloat16 for the bf16 tape); every call runs on torch's current stream.
"""
from __future__ import annotations

import ctypes as C

import torch

from sdp import _lib

P, I, SZ, Fl = C.c_void_p, C.c_int, C.c_size_t, C.c_float
PACK_FRAG, PACK_FRAG16, PACK_DFRAG16, PACK_POOL4X4 = 0, 3, 4, 5


class Conv(C.Structure):
    _fields_ = [("in_", P), ("wf", P), ("wf16", P), ("bias", P), ("out", P), ("res", P), ("out2", P), ("res2", P),
                ("up", P), ("pro_ss", P), ("ss_bstride", I), ("stats", P), ("B", I), ("H", I), ("W", I), ("Cin", I),
                ("Cout", I), ("dil", I), ("circular", I), ("pro_mode", I), ("epi_elu", I), ("aux", P), ("epi_ss", P),
                ("dact", I), ("io16", I), ("s2", I)]


class Wgrad(C.Structure):
    _fields_ = [("in_", P), ("pro_ss", P), ("ss_bstride", I), ("pro_mode", I), ("dy", P), ("part", P),
                ("part_floats", SZ), ("bpart", P), ("B", I), ("H", I), ("W", I), ("Cin", I), ("Cout", I), ("dil", I),
                ("circular", I)]


class Langevin(C.Structure):
    _fields_ = [("x", P), ("ref", P), ("mask", P), ("noise", P), ("seed", C.c_uint64), ("offset", C.c_uint64),
                ("step_size", Fl), ("noise_scale", Fl), ("grad_ref", Fl), ("nan_to_num", I), ("lik_out", P),
                ("absmax_bits", P)]


SIGS = {
    "sdpk_pack_weights": (I, [P, P, I, I, I, I, I, P, P]),
    "sdpk_conv_mfma": (I, [I, C.POINTER(Conv), I, I, P]),
    "sdpk_conv_dgrad": (I, [I, C.POINTER(Conv), I, P]),
    "sdpk_conv_wgrad": (I, [I, C.POINTER(Wgrad), I, P, P, I, I, P]),
    "sdpk_wgrad_splits": (I, [I, I, I, I, I, I, I]),
    "sdpk_wgrad_part_floats": (SZ, [I, I, I, I]),
    "sdpk_maxpool5": (I, [P, P, P, I, I, I, I, I, P]),
    "sdpk_maxpool5_backward": (I, [P, P, P, P, I, I, I, I, I, P]),
    "sdpk_avgpool2": (I, [P, P, I, I, I, I, P]),
    "sdpk_unpool": (I, [P, P, I, I, I, I, I, P]),
    "sdpk_upsample_backward": (I, [P, P, I, I, I, I, I, I, P]),
    "sdpk_elu_backward_post": (I, [P, P, P, P, SZ, I, P]),
    "sdpk_add_tensors": (I, [P, P, P, SZ, I, P]),
    "sdpk_inpp_finalize": (I, [P, I, I, Fl, I, P, P, P, P, P, P, P]),
    "sdpk_inpp_backward": (I, [P, P, P, P, P, I, I, I, P, P, P, P, P, P, P, P, P, I, P]),
    "sdpk_begin_conv": (I, [P, P, P, P, P, I, I, I, I, I, P]),
    "sdpk_end_conv": (I, [P, P, P, P, P, P, P, I, I, I, I, I, I, C.POINTER(Langevin), P]),
    "sdpk_begin_conv_wgrad": (I, [P, P, P, P, P, I, I, I, I, P]),
    "sdpk_end_conv_backward": (I, [P, P, P, P, P, P, P, P, P, P, I, I, I, I, P]),
    "sdpk_head_wgrad_part_floats": (SZ, [I, I, I]),
    "sdpk_range_sky_scan": (I, [P, I, I, P, P, P]),
    "sdpk_block_scan": (I, [P, I, P, P]),
    "sdpk_radix_sort": (I, [P, P, P, P, P, C.c_int64, P, P, I, P]),
}

_bound = None


def lib():
    global _bound
    if _bound is None:
        L = _lib.lib()
        for name, (res, args) in SIGS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _bound = L
    return _bound


class KernelError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        raise KernelError(f"{what}: {lib().sdp_last_error().decode()}")


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def pack_weights(w, mode, packing):
    """w: float32 CUDA [Cout][Cin][k][k] -> the packed 32-bit slots (int32 tensor)."""
    Cout, Cin, k, _ = w.shape
    n = Cout * Cin * (16 if packing == PACK_POOL4X4 else k * k)
    out = torch.empty(n, dtype=torch.int32, device=w.device)
    scratch = torch.empty(64, dtype=torch.uint8, device=w.device)
    check(lib().sdpk_pack_weights(ptr(w), ptr(out), Cout, Cin, k, mode, packing, ptr(scratch), stream()), "pack_weights")
    torch.cuda.synchronize()          # scratch (the launch descriptor) is dropped on return
    return out


def ident_ss(device, n=1024):
    """The identity (scale, shift) = (1, 0) table of the convs without an affine prologue (ss_bstride 0)."""
    return torch.tensor([1.0, 0.0], device=device).repeat(n)
