"""ctypes binding of ``libttship.so`` (the C ABI in ``include/ttship.h``).

The library is built in-tree (``tts_amd/libttship.so``, see ``tts_amd/csrc/Makefile`` and
``__graft_entry__.build``). There is no CPU fallback: if the library or a ROCm device is
missing, every entry point raises ``RuntimeError``.
"""

import atexit
import collections
import ctypes
import os
import threading
from typing import Dict

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TTSHIP_LIB", os.path.join(_HERE, "libttship.so"))

_lib = None
_lock = threading.Lock()

_c_int_p = ctypes.POINTER(ctypes.c_int32)
_c_i64_p = ctypes.POINTER(ctypes.c_int64)
_c_f_p = ctypes.POINTER(ctypes.c_float)
_c_i_p = ctypes.POINTER(ctypes.c_int)
_vp = ctypes.c_void_p

# (name, restype, argtypes) for every symbol declared in include/ttship.h
SIGNATURES = [
    ("tts_version", ctypes.c_int, []),
    ("tts_last_error", ctypes.c_char_p, []),
    ("tts_ctx_create", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    ("tts_ctx_destroy", ctypes.c_int, [_vp]),
    ("tts_taco_set_tensor", ctypes.c_int, [_vp, ctypes.c_char_p, _vp, _c_i64_p, ctypes.c_int]),
    ("tts_taco_finalize", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    ("tts_taco_infer", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_int_p,
                                      ctypes.c_int, ctypes.c_float, _vp, _vp, _vp, _vp, _c_int_p, _c_int_p, _vp]),
    ("tts_taco_infer_spk", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_int_p,
                                          ctypes.c_int, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _c_int_p,
                                          _c_int_p, _vp]),
    ("tts_taco_forward", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _c_int_p,
                                        ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tts_taco_gst_info", ctypes.c_int, [_vp, _c_i_p, _c_i_p, _c_i_p]),
    ("tts_taco_style_mel", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    ("tts_taco_style_tokens", ctypes.c_int, [_vp, _c_int_p, _c_f_p, ctypes.c_int, _vp, _vp]),
    ("tts_taco_infer_style", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_int_p,
                                            ctypes.c_int, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int_p,
                                            _c_int_p, _vp]),
    ("tts_taco_forward_style", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp,
                                              _c_int_p, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tts_taco_mbmelgan_infer", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               _c_int_p, ctypes.c_int, ctypes.c_float, _vp, _vp, _vp, _vp, _vp,
                                               _vp, ctypes.c_int, _vp, _c_int_p, _c_int_p, _vp]),
    ("tts_taco_mbmelgan_submit", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                _c_int_p, ctypes.c_int, ctypes.c_float, _vp, _vp, _vp, _vp, _vp,
                                                _vp, ctypes.c_int, _vp, _c_int_p, _c_int_p, _c_i64_p, _vp]),
    ("tts_taco_mbmelgan_finish", ctypes.c_int, [_vp, ctypes.c_int64, _vp]),
    ("tts_taco_speaker_dim", ctypes.c_int, [_vp, _c_i_p, _c_i_p]),
    ("tts_taco_set_options", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    ("tts_taco_encoder", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    ("tts_taco_postnet", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    ("tts_taco_decoder_state", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tts_tacotron1_set_tensor", ctypes.c_int, [_vp, ctypes.c_char_p, _vp, _c_i64_p, ctypes.c_int]),
    ("tts_tacotron1_finalize", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int]),
    ("tts_tacotron1_infer", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_int_p,
                                           ctypes.c_int, _vp, _vp, _vp, _vp, _c_int_p, _c_int_p, _vp]),
    ("tts_tacotron1_encoder", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    ("tts_tacotron1_postnet", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    ("tts_melgan_set_tensor", ctypes.c_int, [_vp, ctypes.c_char_p, _vp, _c_i64_p, ctypes.c_int]),
    ("tts_melgan_finalize", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_int_p, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int]),
    ("tts_melgan_infer", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    ("tts_melgan_infer_strided", ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _c_int_p,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    ("tts_melgan_generator", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp,
                                            _vp]),
    ("tts_pqmf_synthesis", ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int,
                                          _vp, _vp]),
    ("tts_ge2e_set_tensor", ctypes.c_int, [_vp, ctypes.c_char_p, _vp, _c_i64_p, ctypes.c_int]),
    ("tts_ge2e_finalize", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int]),
    ("tts_ge2e_infer", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    ("tts_pwgan_set_tensor", ctypes.c_int, [_vp, ctypes.c_char_p, _vp, _c_i64_p, ctypes.c_int]),
    ("tts_pwgan_finalize", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _c_int_p, ctypes.c_int]),
    ("tts_pwgan_infer", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp,
                                       _vp]),
    ("tts_glow_set_tensor", ctypes.c_int, [_vp, ctypes.c_char_p, _vp, _c_i64_p, ctypes.c_int]),
    ("tts_glow_finalize", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    ("tts_glow_encode", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, _c_int_p,
                                       _vp]),
    ("tts_glow_encode_spk", ctypes.c_int, [_vp, _vp, _c_int_p, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                           _c_int_p, _vp]),
    ("tts_glow_decode", ctypes.c_int, [_vp, _vp, ctypes.c_float, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    ("tts_glow_align", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("tts_glow_mas", ctypes.c_int, [_vp, _vp, _c_int_p, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    ("tts_time_decoder_kernel", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _c_f_p]),
    ("tts_decoder_stats", ctypes.c_int, [_vp, _c_i_p, _c_i_p, _c_f_p, _c_i_p]),
    ("tts_set_gemm_mode", ctypes.c_int, [_vp, ctypes.c_int]),
    ("tts_test_stall_lstm", ctypes.c_int, [ctypes.c_int]),
    ("tts_test_conv", ctypes.c_int, [_vp, _vp, _vp]),
    ("tts_test_voc", ctypes.c_int, [_vp, _vp, _vp]),
    ("tts_gemm_mode", ctypes.c_int, [_vp, _c_i_p, _c_i64_p]),
    ("tts_mel_to_linear", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         _vp, _vp, _vp, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_float,
                                         ctypes.c_float, _vp, _vp]),
    ("tts_griffin_lim", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    ("tts_stft_mag", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_float, ctypes.c_int, _vp, ctypes.c_int, _vp]),
    ("tts_mag_to_feature", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          _vp, ctypes.c_float, _vp, _vp, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                                          _vp, _vp]),
    ("tts_spec_to_mag", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp,
                                       ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                       _vp, _vp]),
    ("tts_deemphasis", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, _vp, _vp]),
    ("tts_wav_finish", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("tts_pqmf_analysis", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp,
                                         ctypes.c_int, _vp, ctypes.c_int, _vp]),
    ("tts_stft_pair_sums", ctypes.c_int, [_vp, _vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, _vp, _vp]),
    ("tts_torch_stft_mag", ctypes.c_int, [_vp, _vp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, _vp, ctypes.c_int, _vp]),
]


class ConvTest(ctypes.Structure):
    """``tts_conv_test`` of include/ttship.h (the descriptor of tts_test_conv)."""
    _fields_ = [
        ("h_weight", _vp), ("h_bias", _vp),
        ("transposed", ctypes.c_int32), ("Cin", ctypes.c_int32), ("Cout", ctypes.c_int32), ("K", ctypes.c_int32),
        ("dil", ctypes.c_int32), ("nphase", ctypes.c_int32),
        ("pad_left", ctypes.c_int32 * 8),
        ("merged_u", ctypes.c_int32), ("nsrc", ctypes.c_int32),
        ("d_src", _vp * 2),
        ("src_strides", (ctypes.c_int64 * 3) * 2),
        ("src_C", ctypes.c_int32 * 2), ("src_act", ctypes.c_int32 * 2),
        ("d_out", _vp), ("out_strides", ctypes.c_int64 * 3),
        ("d_resid", _vp), ("resid_strides", ctypes.c_int64 * 3), ("resid_rows", ctypes.c_int32),
        ("d_aux", _vp), ("auxb", ctypes.c_int64),
        ("h_lens", _vp),
        ("B", ctypes.c_int32), ("max_q", ctypes.c_int32), ("len_add", ctypes.c_int32), ("in_mul", ctypes.c_int32),
        ("q_mul", ctypes.c_int32), ("out_mul", ctypes.c_int32), ("rep_pad", ctypes.c_int32),
        ("pad_mode", ctypes.c_int32), ("epi", ctypes.c_int32),
        ("ran_x3", ctypes.c_int32), ("tq", ctypes.c_int32), ("range_flag", ctypes.c_uint32),
    ]


class VocTest(ctypes.Structure):
    """``tts_voc_test`` of include/ttship.h (the descriptor of tts_test_voc)."""
    _fields_ = [
        ("kind", ctypes.c_int32), ("C", ctypes.c_int32), ("N", ctypes.c_int32), ("taps", ctypes.c_int32),
        ("wd", _vp * 3), ("bd", _vp * 3), ("w1", _vp * 3), ("b1", _vp * 3), ("ws", _vp * 3), ("bs", _vp * 3),
        ("dil", ctypes.c_int32 * 3),
        ("ct_w", _vp), ("ct_b", _vp), ("wo", _vp), ("bo", _vp), ("G", _vp),
        ("d_x", _vp), ("d_y", _vp),
        ("x_strides", ctypes.c_int64 * 2), ("y_strides", ctypes.c_int64 * 2),
        ("h_lens", _vp), ("h_bounds", _vp),
        ("B", ctypes.c_int32), ("len_add", ctypes.c_int32), ("mul", ctypes.c_int32), ("max_q", ctypes.c_int32),
        ("tq", ctypes.c_int32), ("range_flag", ctypes.c_uint32),
    ]


def load_library():
    """Load and type the shared library (no GPU calls are made here)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(f"libttship.so not found at {LIB_PATH}; run __graft_entry__.build() "
                                   f"(make -C tts_amd/csrc)")
            lib = ctypes.CDLL(LIB_PATH)
            for name, res, args in SIGNATURES:
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def _check(rc: int):
    if rc != 0:
        msg = load_library().tts_last_error()
        raise RuntimeError("ttship: " + (msg.decode() if msg else "unknown error"))


def _i32(a):
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.int32))
    return arr, arr.ctypes.data_as(_c_int_p)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _opt_ptr(t):
    return None if t is None else _ptr(t)


def _stream(device):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Engine:
    """One library context per device (owns packed weights, workspace, captured graphs)."""

    def __init__(self, device_index: int):
        self.lib = load_library()
        self.device = device_index
        # Held by every model across its weight check-and-upload (``_sync``) and its whole compute
        # sequence: the context's workspace, graphs and packed weights are shared by all models on
        # this device, and ctypes releases the GIL inside each call. (Each C entry point also locks
        # the context; this lock makes multi-call sequences such as Glow encode + decode atomic.)
        self.lock = threading.RLock()
        self._live = collections.OrderedDict()  # ticket -> (post, wav) of unfinished fused submissions
        h = ctypes.c_void_p()
        _check(self.lib.tts_ctx_create(device_index, ctypes.byref(h)))
        self.h = h
        self.weight_keys = {}  # weight slot -> (token, version) of the model whose weights it holds

    def close(self):
        if self.h:
            self.lib.tts_ctx_destroy(self.h)
            self.h = None

    # -- weights ---------------------------------------------------------------------
    def _set(self, fn, name, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        shape = (ctypes.c_int64 * max(1, a.ndim))(*a.shape)
        _check(fn(self.h, name.encode(), a.ctypes.data_as(ctypes.c_void_p), shape, a.ndim))

    def _load_model(self, prefix, tensors, *finalize_args):
        set_tensor = getattr(self.lib, f"tts_{prefix}_set_tensor")
        for k, v in tensors.items():
            self._set(set_tensor, k, v)
        _check(getattr(self.lib, f"tts_{prefix}_finalize")(self.h, *finalize_args))

    def load_tacotron(self, tensors: Dict[str, np.ndarray], num_chars: int, r_init: int, attn_norm: str,
                      windowing: bool = False, forward_attn: bool = False, forward_attn_mask: bool = False):
        _check(self.lib.tts_taco_set_options(self.h, int(bool(windowing)), int(bool(forward_attn)),
                                             int(bool(forward_attn and forward_attn_mask))))
        self._load_model("taco", tensors, num_chars, r_init, 1 if attn_norm == "softmax" else 0)

    def load_melgan(self, tensors: Dict[str, np.ndarray], in_channels, out_channels, base_channels,
                    upsample_factors, num_res_blocks, use_pqmf):
        ups, ups_p = _i32(list(upsample_factors))
        self._load_model("melgan", tensors, in_channels, out_channels, base_channels, ups_p, len(ups),
                         num_res_blocks, 1 if use_pqmf else 0)

    # -- compute (device tensors) ----------------------------------------------------
    def _decode_args(self, ids, lens, r, max_steps, S_cap):
        """What the Tacotron decode entry points share: their leading arguments, the per-row steps /
        status arrays they fill with the pointers to them, and the host arrays behind the leading
        pointers (the caller holds on to those until the call has returned)."""
        B, T = ids.shape
        lens_a, lens_p = _i32(lens)
        ms_a, ms_p = _i32(max_steps)
        steps = np.zeros(B, np.int32)
        status = np.zeros(B, np.int32)
        return ((self.h, _ptr(ids), lens_p, B, T, r, ms_p, S_cap), steps, status,
                (steps.ctypes.data_as(_c_int_p), status.ctypes.data_as(_c_int_p)), (lens_a, ms_a))

    def taco_infer(self, ids, lens, r, max_steps, S_cap, stop_threshold, dec, post, align, stop,
                   speaker_ids=None, speaker_embeddings=None, style=None):
        """``style``: (B, gst_dim) style vectors of a GST model (tts_taco_infer_style), None = zeros."""
        head, steps, status, res, keep = self._decode_args(ids, lens, r, max_steps, S_cap)
        outs = (_ptr(dec), _ptr(post), _ptr(align), _ptr(stop))
        if style is not None:
            _check(self.lib.tts_taco_infer_style(*head, float(stop_threshold), _opt_ptr(speaker_ids),
                                                 _opt_ptr(speaker_embeddings), _ptr(style), *outs, *res,
                                                 _stream(ids.device)))
        elif speaker_ids is None and speaker_embeddings is None:
            _check(self.lib.tts_taco_infer(*head, float(stop_threshold), *outs, *res, _stream(ids.device)))
        else:
            _check(self.lib.tts_taco_infer_spk(*head, float(stop_threshold), _opt_ptr(speaker_ids),
                                               _opt_ptr(speaker_embeddings), *outs, *res, _stream(ids.device)))
        return steps, status

    def taco_forward(self, ids, lens, r, mel, mel_lens, dec, post, align, stop, speaker_ids=None,
                     speaker_embeddings=None, style=None):
        """Teacher-forced Tacotron2.forward in eval (tts_taco_forward): ``mel`` (B, M, 80) contiguous
        fp32 with M a multiple of r; dec / post (B, M, 80), align (B, M / r, T), stop (B, M / r).
        ``style``: (B, gst_dim) style vectors of a GST model (tts_taco_forward_style)."""
        B, T = ids.shape
        lens_a, lens_p = _i32(lens)
        ml_a, ml_p = _i32(mel_lens)
        head = (self.h, _ptr(ids), lens_p, B, T, r, _ptr(mel), ml_p, int(mel.shape[1]), _opt_ptr(speaker_ids),
                _opt_ptr(speaker_embeddings))
        tail = (_ptr(dec), _ptr(post), _ptr(align), _ptr(stop), _stream(ids.device))
        if style is not None:
            _check(self.lib.tts_taco_forward_style(*head, _ptr(style), *tail))
        else:
            _check(self.lib.tts_taco_forward(*head, *tail))

    def taco_gst_info(self):
        """(gst_dim, num_tokens, query_uses_speaker) of the loaded Tacotron2 (tts_taco_gst_info)."""
        g, n, q = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _check(self.lib.tts_taco_gst_info(self.h, ctypes.byref(g), ctypes.byref(n), ctypes.byref(q)))
        return g.value, n.value, bool(q.value)

    def taco_style_mel(self, mel, lens, speaker_embeddings, style):
        """Style vectors of mels (tts_taco_style_mel): ``mel`` (B, N, 80) contiguous fp32, ``lens`` the
        rows' frame counts, ``speaker_embeddings`` (B, Es) or None -> ``style`` (B, gst_dim)."""
        B, N, _ = mel.shape
        lens_a, lens_p = _i32(lens)
        _check(self.lib.tts_taco_style_mel(self.h, _ptr(mel), lens_p, B, N, _opt_ptr(speaker_embeddings),
                                           _ptr(style), _stream(mel.device)))

    def taco_style_tokens(self, token_ids, weights, style):
        """Style vector of a {token: weight} dict (tts_taco_style_tokens) -> ``style`` (gst_dim)."""
        ids_a, ids_p = _i32(token_ids)
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32))
        _check(self.lib.tts_taco_style_tokens(self.h, ids_p, w.ctypes.data_as(_c_f_p), len(ids_a), _ptr(style),
                                              _stream(style.device)))

    def taco_mbmelgan_infer(self, ids, lens, r, max_steps, S_cap, stop_threshold, dec, post, align, stop, pad, wav,
                            speaker_ids=None, speaker_embeddings=None):
        """Tacotron2 decode and MB-MelGAN on its postnet output in one library call
        (tts_taco_mbmelgan_infer); ``wav`` holds B * hop * (S_cap * r + 2 pad) floats."""
        head, steps, status, res, keep = self._decode_args(ids, lens, r, max_steps, S_cap)
        _check(self.lib.tts_taco_mbmelgan_infer(*head, float(stop_threshold), _opt_ptr(speaker_ids),
                                                _opt_ptr(speaker_embeddings), _ptr(dec), _ptr(post), _ptr(align),
                                                _ptr(stop), int(pad), _ptr(wav), *res, _stream(ids.device)))
        return steps, status

    def taco_mbmelgan_submit(self, ids, lens, r, max_steps, S_cap, stop_threshold, dec, post, align, stop, pad, wav,
                             speaker_ids=None, speaker_embeddings=None):
        """The first half of taco_mbmelgan_infer (tts_taco_mbmelgan_submit): returns (steps, status,
        ticket) once the decode is done, the vocoder still running; ``post`` and ``wav`` must stay
        untouched until ``taco_mbmelgan_finish(ticket)``."""
        head, steps, status, res, keep = self._decode_args(ids, lens, r, max_steps, S_cap)
        ticket = ctypes.c_int64(0)
        _check(self.lib.tts_taco_mbmelgan_submit(*head, float(stop_threshold), _opt_ptr(speaker_ids),
                                                 _opt_ptr(speaker_embeddings), _ptr(dec), _ptr(post), _ptr(align),
                                                 _ptr(stop), int(pad), _ptr(wav), *res, ctypes.byref(ticket),
                                                 _stream(ids.device)))
        # a fp32 re-run at finish reads post and writes wav: keep them allocated while the library
        # may still do that (it finishes a ticket at the latest when the 5th submission after it
        # reuses its slot)
        self._live[ticket.value] = (post, wav)
        while len(self._live) > 4:
            self._live.popitem(last=False)
        return steps, status, ticket.value

    def taco_mbmelgan_finish(self, ticket, device):
        """Completes a submission (tts_taco_mbmelgan_finish): its waveforms are final after this."""
        _check(self.lib.tts_taco_mbmelgan_finish(self.h, int(ticket), _stream(device)))
        self._live.pop(int(ticket), None)

    def taco_speaker_dim(self):
        d, n = ctypes.c_int(0), ctypes.c_int(0)
        _check(self.lib.tts_taco_speaker_dim(self.h, ctypes.byref(d), ctypes.byref(n)))
        return d.value, n.value

    def taco_encoder(self, ids, lens, out):
        B, T = ids.shape
        lens_a, lens_p = _i32(lens)
        _check(self.lib.tts_taco_encoder(self.h, _ptr(ids), lens_p, B, T, _ptr(out), _stream(ids.device)))

    def taco_postnet(self, dec, lens, out):
        B, M, _ = dec.shape
        lens_a, lens_p = _i32(lens)
        _check(self.lib.tts_taco_postnet(self.h, _ptr(dec), lens_p, B, M, _ptr(out), _stream(dec.device)))

    def taco_decoder_state(self, B, T_max, device, key=None):
        """Decoder state after the last Tacotron2 decode (tts_taco_decoder_state), caller row order.
        ``key``: the calling model's weight key; the read is refused if another model (or another
        version of this one) decoded on this device since."""
        import torch
        out = {k: torch.empty(B, n, device=device) for k, n in
               (("query", 1024), ("attention_rnn_cell_state", 1024), ("decoder_hidden", 1024),
                ("decoder_cell", 1024), ("context", 512), ("attention_weights", T_max),
                ("attention_weights_cum", T_max))}
        with self.lock:
            if key is not None and self.weight_keys.get("taco") != key:
                raise RuntimeError("decoder_state: another Tacotron2 model decoded on this device since this model's call")
            _check(self.lib.tts_taco_decoder_state(self.h, B, T_max, *[_ptr(out[k]) for k in out], _stream(device)))
        return out

    def load_tacotron1(self, tensors: Dict[str, np.ndarray], num_chars, r_init, memory_size, attn_norm,
                       postnet_output_dim):
        self._load_model("tacotron1", tensors, num_chars, r_init, memory_size, 1 if attn_norm == "softmax" else 0,
                         postnet_output_dim)

    def tacotron1_infer(self, ids, lens, r, max_steps, S_cap, dec, post, align, stop):
        """Batched Tacotron.inference (tts_tacotron1_infer); S_cap > max(max_steps)."""
        head, steps, status, res, keep = self._decode_args(ids, lens, r, max_steps, S_cap)
        _check(self.lib.tts_tacotron1_infer(*head, _ptr(dec), _ptr(post), _ptr(align), _ptr(stop), *res,
                                            _stream(ids.device)))
        return steps, status

    def tacotron1_encoder(self, ids, lens, out):
        B, T = ids.shape
        lens_a, lens_p = _i32(lens)
        _check(self.lib.tts_tacotron1_encoder(self.h, _ptr(ids), lens_p, B, T, _ptr(out), _stream(ids.device)))

    def tacotron1_postnet(self, dec, lens, out):
        B, M, _ = dec.shape
        lens_a, lens_p = _i32(lens)
        _check(self.lib.tts_tacotron1_postnet(self.h, _ptr(dec), lens_p, B, M, _ptr(out), _stream(dec.device)))

    def load_pwgan(self, tensors: Dict[str, np.ndarray], num_res_blocks, stacks, upsample_factors):
        ups, ups_p = _i32(list(upsample_factors))
        self._load_model("pwgan", tensors, num_res_blocks, stacks, ups_p, len(ups))

    def pwgan_infer(self, mel, lens, pad, noise, out):
        B, _, M = mel.shape
        lens_a, lens_p = _i32(lens)
        _check(self.lib.tts_pwgan_infer(self.h, _ptr(mel), lens_p, B, M, pad, _ptr(noise), _ptr(out),
                                        _stream(mel.device)))

    def load_glow(self, tensors: Dict[str, np.ndarray], num_chars, enc_layers, flows, wn_layers):
        self._load_model("glow", tensors, num_chars, enc_layers, flows, wn_layers)

    def glow_encode(self, ids, lens, length_scale, speaker_ids=None):
        B, T = ids.shape
        lens_a, lens_p = _i32(lens)
        ylens = np.zeros(B, np.int32)
        if speaker_ids is None:
            _check(self.lib.tts_glow_encode(self.h, _ptr(ids), lens_p, B, T, float(length_scale),
                                            ylens.ctypes.data_as(_c_int_p), _stream(ids.device)))
        else:
            spk_a, spk_p = _i32(speaker_ids)
            if len(spk_a) != B:
                raise ValueError("one speaker id per utterance")
            _check(self.lib.tts_glow_encode_spk(self.h, _ptr(ids), lens_p, spk_p, B, T, float(length_scale),
                                                ylens.ctypes.data_as(_c_int_p), _stream(ids.device)))
        return ylens

    def glow_decode(self, noise, noise_scale, Ty, y, y_mean, attn, logw):
        _check(self.lib.tts_glow_decode(self.h, _ptr(noise), float(noise_scale), Ty, _ptr(y), _ptr(y_mean),
                                        _ptr(attn), _ptr(logw), _stream(y.device)))

    def glow_align(self, y, ylens, z, logdet, logp, attn, y_mean, o_attn_dur, logw):
        """GlowTts.forward after glow_encode of the same batch; ``logp`` may be None."""
        yl_a, yl_p = _i32(ylens)
        _check(self.lib.tts_glow_align(self.h, _ptr(y), yl_p, int(y.shape[2]), _ptr(z), _ptr(logdet),
                                       _opt_ptr(logp), _ptr(attn), _ptr(y_mean),
                                       _ptr(o_attn_dur), _ptr(logw), _stream(y.device)))

    def glow_mas(self, logp, xlens, ylens):
        """maximum_path on the device: logp (B, Tx, Ty) float32 -> path (B, Tx, Ty) of 0 / 1."""
        B, Tx, Ty = logp.shape
        import torch
        xl_a, xl_p = _i32(xlens)
        yl_a, yl_p = _i32(ylens)
        path = torch.empty_like(logp)
        _check(self.lib.tts_glow_mas(self.h, _ptr(logp), xl_p, yl_p, B, Tx, Ty, _ptr(path), _stream(logp.device)))
        return path

    def load_ge2e(self, tensors: Dict[str, np.ndarray], input_dim, proj_dim, lstm_dim, num_layers, with_proj):
        self._load_model("ge2e", tensors, input_dim, proj_dim, lstm_dim, num_layers, 1 if with_proj else 0)

    def ge2e_infer(self, x, lens, out):
        B, T, _ = x.shape
        lens_a, lens_p = _i32(lens)
        _check(self.lib.tts_ge2e_infer(self.h, _ptr(x), lens_p, B, T, _ptr(out), _stream(x.device)))

    def melgan_infer(self, mel, lens, pad, wav):
        """mel (B, C, M): contiguous, or any strided view the library reads in place (e.g. a
        (B, M, C) postnet output transposed)."""
        B, _, M = mel.shape
        lens_a, lens_p = _i32(lens)
        if mel.is_contiguous():
            _check(self.lib.tts_melgan_infer(self.h, _ptr(mel), lens_p, B, M, pad, _ptr(wav), _stream(mel.device)))
        else:
            sb, sc, st = mel.stride()
            _check(self.lib.tts_melgan_infer_strided(self.h, _ptr(mel), sb, sc, st, lens_p, B, M, pad, _ptr(wav),
                                                     _stream(mel.device)))

    def melgan_generator(self, mel, lens, pad, out):
        B, _, M = mel.shape
        lens_a, lens_p = _i32(lens)
        _check(self.lib.tts_melgan_generator(self.h, _ptr(mel), lens_p, B, M, pad, _ptr(out),
                                             _stream(mel.device)))

    def pqmf_synthesis(self, x, G, y):
        B, N, L = x.shape
        taps = G.shape[-1] - 1
        _check(self.lib.tts_pqmf_synthesis(self.h, _ptr(x), B, N, L, _ptr(G), taps, _ptr(y), _stream(x.device)))

    def mel_to_linear(self, mel, lens, inv_basis, scale, offset, clip, spec_gain, power, S):
        """Normalised mel (B, M, n_mels) -> linear magnitudes ``S`` (B, M, n_freq) (tts_mel_to_linear);
        ``clip`` is None or the (lo, hi) bounds applied to the mel before denormalising."""
        B, M, n_mels = mel.shape
        lens_a, lens_p = _i32(lens)
        lo, hi = (0.0, 0.0) if clip is None else clip
        _check(self.lib.tts_mel_to_linear(self.h, _ptr(mel), lens_p, B, M, n_mels, S.shape[-1], _ptr(inv_basis),
                                          _ptr(scale), _ptr(offset), float(lo), float(hi), int(clip is not None),
                                          float(spec_gain), float(power), _ptr(S), _stream(mel.device)))

    def griffin_lim(self, S, lens, n_fft, win_length, hop_length, iters, phase0, wav):
        """Batched Griffin-Lim (tts_griffin_lim): magnitudes ``S`` and uniform [0, 1) ``phase0``
        (B, M, n_fft / 2 + 1) -> ``wav`` (B, hop_length * (M - 1))."""
        B, M, _ = S.shape
        lens_a, lens_p = _i32(lens)
        _check(self.lib.tts_griffin_lim(self.h, _ptr(S), lens_p, B, M, int(n_fft), int(win_length), int(hop_length),
                                        int(iters), _ptr(phase0), _ptr(wav), _stream(S.device)))

    def stft_mag(self, wav, nsamples, n_fft, win_length, hop_length, preemphasis, mag, algo=0):
        """Batched STFT magnitudes (tts_stft_mag): ``wav`` (B, L_max) with ``nsamples[b]`` valid
        samples per row -> ``mag`` (B, M_max, n_fft / 2 + 1), row b zero past 1 + nsamples[b] //
        hop_length frames. ``algo``: 0 auto, 1 the 1024-point FFT kernel, 2 the direct DFT."""
        B, L = wav.shape
        n_a, n_p = _i32(nsamples)
        _check(self.lib.tts_stft_mag(self.h, _ptr(wav), n_p, B, L, int(n_fft), int(win_length), int(hop_length),
                                     float(preemphasis), int(algo), _ptr(mag), mag.shape[1], _stream(wav.device)))

    def mag_to_feature(self, mag, lens, basis, spec_gain, scale, offset, clip, out):
        """Magnitudes (B, M, n_freq) -> normalised dB features ``out`` (B, M, n_out)
        (tts_mag_to_feature); ``basis`` (n_out, n_freq) or None (linear spectrogram), ``clip`` None
        or the (lo, hi) bounds applied to the result."""
        B, M, n_freq = mag.shape
        lens_a, lens_p = _i32(lens)
        lo, hi = (0.0, 0.0) if clip is None else clip
        _check(self.lib.tts_mag_to_feature(self.h, _ptr(mag), lens_p, B, M, n_freq, out.shape[-1],
                                           None if basis is None else _ptr(basis), float(spec_gain), _ptr(scale),
                                           _ptr(offset), float(lo), float(hi), int(clip is not None), _ptr(out),
                                           _stream(mag.device)))

    def spec_to_mag(self, spec, lens, scale, offset, clip, spec_gain, power, S):
        """Normalised linear spectrograms (B, M, n_freq) -> magnitudes ``S``, the same shape
        (tts_spec_to_mag); ``clip`` as in `mel_to_linear`."""
        B, M, n_freq = spec.shape
        lens_a, lens_p = _i32(lens)
        lo, hi = (0.0, 0.0) if clip is None else clip
        _check(self.lib.tts_spec_to_mag(self.h, _ptr(spec), lens_p, B, M, n_freq, _ptr(scale), _ptr(offset),
                                        float(lo), float(hi), int(clip is not None), float(spec_gain), float(power),
                                        _ptr(S), _stream(spec.device)))

    def deemphasis(self, wav, nsamples, a, out):
        """y[n] = x[n] + a y[n-1] on every row of ``wav`` (B, L_max) for ``nsamples[b]`` samples
        (tts_deemphasis); ``out`` may be ``wav``, and is zero past each row's count."""
        B, L = wav.shape
        n_a, n_p = _i32(nsamples)
        _check(self.lib.tts_deemphasis(self.h, _ptr(wav), n_p, B, L, float(a), _ptr(out), _stream(wav.device)))

    def wav_finish(self, wav, nsamples, window_length, hop_length, threshold, gap, pcm, ends, total):
        """Endpoints, join with gaps and 16-bit scaling of ``wav`` (B, L_max) (tts_wav_finish) into
        the device tensors ``pcm`` (int16), ``ends`` (B int32) and ``total`` (one int32)."""
        B, L = wav.shape
        n_a, n_p = _i32(nsamples)
        _check(self.lib.tts_wav_finish(self.h, _ptr(wav), n_p, B, L, int(window_length), int(hop_length),
                                       float(threshold), int(gap), _ptr(pcm), _ptr(ends), _ptr(total),
                                       _stream(wav.device)))

    def pqmf_analysis(self, x, lens, H, y):
        """PQMF.analysis (tts_pqmf_analysis): ``x`` (B, L_max) with ``lens[b]`` valid samples per row,
        ``H`` (N, taps + 1) -> ``y`` (B, N, Lout_max), row b zero past (lens[b] - 1) // N + 1."""
        B, L = x.shape
        l_a, l_p = _i32(lens)
        _check(self.lib.tts_pqmf_analysis(self.h, _ptr(x), l_p, B, L, H.shape[0], _ptr(H), H.shape[1] - 1, _ptr(y),
                                          y.shape[2], _stream(x.device)))

    def stft_pair_sums(self, y_hat, y, nsamples, n_fft, win_length, hop_length, sums):
        """Per-row STFT distance sums of one resolution (tts_stft_pair_sums): ``y_hat``, ``y``
        (B, L_max) with ``nsamples[b]`` valid samples per row -> ``sums`` (B, 3) float64:
        sum |log y_M - log y_hat_M|, sum (y_M - y_hat_M)^2, sum y_M^2."""
        B, L = y.shape
        n_a, n_p = _i32(nsamples)
        _check(self.lib.tts_stft_pair_sums(self.h, _ptr(y_hat), _ptr(y), n_p, B, L, int(n_fft), int(win_length),
                                           int(hop_length), _ptr(sums), _stream(y.device)))

    def torch_stft_mag(self, wav, nsamples, n_fft, win_length, hop_length, mag):
        """TorchSTFT magnitudes (tts_torch_stft_mag): ``wav`` (B, L_max) -> ``mag``
        (B, n_fft // 2 + 1, frames_max), row b zero past its own frames."""
        B, L = wav.shape
        n_a, n_p = _i32(nsamples)
        _check(self.lib.tts_torch_stft_mag(self.h, _ptr(wav), n_p, B, L, int(n_fft), int(win_length),
                                           int(hop_length), _ptr(mag), mag.shape[2], _stream(wav.device)))

    def conv_test(self, weight, bias, lens, src, out, max_q, device, transposed=False, K=1, dil=1, nphase=1,
                  pad_left=(0,), merged_u=0, src2=None, resid=None, resid_rows=0, aux=None, auxb=0, len_add=0,
                  in_mul=1, q_mul=1, out_mul=1, rep_pad=0, pad_mode=0, epi=0):
        """One generic conv launch through pack_conv / run_conv (tts_test_conv; tests and tools).
        ``weight``: numpy (Cout, Cin, K), (nphase, Cout, Cin, K), or (Cin, Cout, 2 nphase) when
        ``transposed``; ``src`` / ``src2``: (device address, (sb, sc, st), channels, act); ``out`` /
        ``resid``: (device address, (sb, sc, st)); ``aux``: device address. Returns (ran_x3, tq,
        range_flag)."""
        w = np.ascontiguousarray(weight, dtype=np.float32)
        b = np.ascontiguousarray(bias, dtype=np.float32)
        lens_a = np.ascontiguousarray(lens, dtype=np.int32)
        d = ConvTest()
        d.h_weight, d.h_bias, d.h_lens = w.ctypes.data, b.ctypes.data, lens_a.ctypes.data
        d.transposed = int(bool(transposed))
        if transposed:
            d.Cin, d.Cout = w.shape[0], w.shape[1]
        else:
            d.Cout, d.Cin = w.shape[-3], w.shape[-2]
        assert len(b) == d.Cout
        d.K, d.dil, d.nphase, d.merged_u = K, dil, nphase, merged_u
        for i, p in enumerate(pad_left):
            d.pad_left[i] = p
        d.nsrc = 1 if src2 is None else 2
        for i, s in enumerate((src,) if src2 is None else (src, src2)):
            d.d_src[i] = s[0]
            for j in range(3):
                d.src_strides[i][j] = s[1][j]
            d.src_C[i], d.src_act[i] = s[2], s[3]
        d.d_out = out[0]
        for j in range(3):
            d.out_strides[j] = out[1][j]
        if resid is not None:
            d.d_resid = resid[0]
            for j in range(3):
                d.resid_strides[j] = resid[1][j]
        d.resid_rows, d.d_aux, d.auxb = resid_rows, aux, auxb
        d.B, d.max_q, d.len_add, d.in_mul, d.q_mul, d.out_mul = len(lens_a), max_q, len_add, in_mul, q_mul, out_mul
        d.rep_pad, d.pad_mode, d.epi = rep_pad, pad_mode, epi
        with self.lock:
            _check(self.lib.tts_test_conv(self.h, ctypes.c_void_p(ctypes.addressof(d)), _stream(device)))
        return bool(d.ran_x3), int(d.tq), int(d.range_flag)

    def voc_test(self, kind, C, lens, x, y, max_q, device, blocks=(), ct=None, out=None, G=None, bounds=None,
                 len_add=0, mul=1):
        """One vocoder kernel launch through the loaders' packing (tts_test_voc; tests and tools).
        ``kind``: 0 resblock fp32, 1 resblock_x3, 2 resstack_x3, 3 resstack_x3 with the fused
        ConvTranspose, 4 output conv + PQMF, 5 full-band output conv. ``blocks``: per block
        (wd, bd, w1, b1, ws, bs, dil) as numpy; ``ct``: (ct_w, ct_b); ``out``: (wo, bo); ``G``: the PQMF
        synthesis filter (N, taps + 1); ``x`` / ``y``: (device address, (batch stride, channel stride));
        ``bounds``: the launcher's host lengths when they are upper bounds of ``lens``. Returns
        (tq, range_flag)."""
        keep = []

        def f32(a):
            a = np.ascontiguousarray(a, dtype=np.float32)
            keep.append(a)
            return a.ctypes.data

        d = VocTest()
        d.kind, d.C = int(kind), int(C)
        for k, blk in enumerate(blocks):
            wd, bd, w1, b1, ws, bs, dil = blk
            assert np.shape(wd) == (C, C, 3) and np.size(w1) == C * C and np.size(ws) == C * C
            assert np.size(bd) == C and np.size(b1) == C and np.size(bs) == C
            d.wd[k], d.bd[k], d.w1[k], d.b1[k], d.ws[k], d.bs[k] = f32(wd), f32(bd), f32(w1), f32(b1), f32(ws), f32(bs)
            d.dil[k] = int(dil)
        if ct is not None:
            assert np.shape(ct[0]) == (2 * C, C, 4) and np.size(ct[1]) == C
            d.ct_w, d.ct_b = f32(ct[0]), f32(ct[1])
        if out is not None:
            d.N = int(np.shape(out[0])[0])
            assert np.shape(out[0]) == (d.N, C, 7) and np.size(out[1]) == d.N
            d.wo, d.bo = f32(out[0]), f32(out[1])
        if G is not None:
            assert np.ndim(G) == 2 and np.shape(G)[0] == d.N
            d.taps = int(np.shape(G)[1]) - 1
            d.G = f32(G)
        lens_a = np.ascontiguousarray(lens, dtype=np.int32)
        d.h_lens = lens_a.ctypes.data
        if bounds is not None:
            bounds_a = np.ascontiguousarray(bounds, dtype=np.int32)
            assert bounds_a.shape == lens_a.shape
            d.h_bounds = bounds_a.ctypes.data
        d.d_x, d.d_y = x[0], y[0]
        for j in range(2):
            d.x_strides[j], d.y_strides[j] = x[1][j], y[1][j]
        d.B, d.len_add, d.mul, d.max_q = len(lens_a), int(len_add), int(mul), int(max_q)
        with self.lock:
            _check(self.lib.tts_test_voc(self.h, ctypes.c_void_p(ctypes.addressof(d)), _stream(device)))
        return int(d.tq), int(d.range_flag)

    def decoder_stats(self):
        """(path, [(ms, steps) per persistent launch]) of the last Tacotron2 decode."""
        path, n = ctypes.c_int(0), ctypes.c_int(0)
        ms = (ctypes.c_float * 4)()   # up to 4 persistent launches (batch tiles of 64, 48, 32, 16 rows)
        st = (ctypes.c_int * 4)()
        _check(self.lib.tts_decoder_stats(self.h, ctypes.byref(path), ctypes.byref(n), ms, st))
        return int(path.value), [(float(ms[i]), int(st[i])) for i in range(n.value)]

    def set_gemm_mode(self, mode: str):
        """'x3' = split-f16 MFMA GEMMs where built (fp32-accurate, the default), 'f32' = fp32 MFMA."""
        if mode not in ("x3", "f32"):
            raise ValueError("gemm mode must be 'x3' or 'f32'")
        with self.lock:
            _check(self.lib.tts_set_gemm_mode(self.h, 1 if mode == "x3" else 0))

    def gemm_mode(self):
        """(mode, calls re-run in fp32 because an operand left the f16 range)."""
        m, n = ctypes.c_int(0), ctypes.c_int64(0)
        _check(self.lib.tts_gemm_mode(self.h, ctypes.byref(m), ctypes.byref(n)))
        return ("x3" if m.value else "f32"), int(n.value)

    def time_decoder_kernel(self, which: int, iters: int) -> float:
        ms = ctypes.c_float(0.0)
        _check(self.lib.tts_time_decoder_kernel(self.h, which, iters, ctypes.byref(ms)))
        return float(ms.value)


_engines: Dict[int, Engine] = {}


def get_engine(device) -> Engine:
    """Engine for a torch device (must be a ROCm 'cuda' device)."""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("tts_amd runs on MI355X (ROCm 'cuda' devices) only; got device "
                           f"'{dev}'. There is no CPU fallback: move the model with .cuda().")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with _lock:
        eng = _engines.get(idx)
    if eng is None:
        eng = Engine(idx)
        with _lock:
            _engines[idx] = eng
    return eng


@atexit.register
def _close_engines():
    """Destroy every context (graphs, streams, device buffers) before interpreter teardown, so the
    HIP runtime and any attached tool (rocprofv3) never see leaked objects after finalisation."""
    with _lock:
        engines = list(_engines.values())
        _engines.clear()
    for eng in engines:
        try:
            eng.close()
        except Exception:
            pass
