"""ctypes binding of ``libseld_hip.so`` (C ABI: ``include/seld_hip.h``).

PyTorch is used for device memory and streams only; every entry point below hands raw
device pointers (``tensor.data_ptr()``) and the current HIP stream to the hand-written
gfx950 kernels.  There is NO CPU fallback: if the shared library is missing or a GPU call
fails, a ``RuntimeError`` is raised.
"""
from __future__ import annotations

import ctypes
import os
import threading
from pathlib import Path

import torch

# SELD_AUGMENT_PARAM_INTS (pattern, 2 x (time start, length), 2 x (frequency start, length), azimuth step, padding) and
# SELD_AUGMENT_PATTERNS: defined once, in seld_augment (numpy only, so no import cycle)
from seld_augment import PARAM_INTS as AUGMENT_PARAM_INTS, PATTERNS as AUGMENT_PATTERNS, check_channel_order
from seld_augment import SPECTRAL_PARAM_INTS          # SELD_SPECTRAL_PARAM_INTS: the spectral row of csrc/spectral.hip

_HERE = Path(__file__).resolve().parent
# SELD_HIP_LIB: developer override to load an experimental build of the SAME library (A/B kernel experiments)
LIB_PATH = Path(os.environ["SELD_HIP_LIB"]).resolve() if os.environ.get("SELD_HIP_LIB") else _HERE / "libseld_hip.so"

N_FFT = 960
HOP = 480
N_BINS = 481
N_MELS = 64

_lock = threading.Lock()
_lib = None
_initialised_devices = set()

_i64 = ctypes.c_int64
_int = ctypes.c_int
_ptr = ctypes.c_void_p


class SeldNativeError(RuntimeError):
    pass


def _declare(lib):
    lib.seld_last_error.restype = ctypes.c_char_p
    lib.seld_last_error.argtypes = []
    lib.seld_version.restype = _int
    lib.seld_version.argtypes = []
    lib.seld_init.argtypes = [_int]
    lib.seld_shutdown.argtypes = []
    lib.seld_num_cus.restype = _int
    lib.seld_num_cus.argtypes = []
    lib.seld_set_mel_filterbank.argtypes = [_ptr]
    lib.seld_set_window.argtypes = [_ptr]
    lib.seld_default_tables.argtypes = [_ptr] * 5
    lib.seld_num_frames.restype = _i64
    lib.seld_num_frames.argtypes = [_i64]
    for name in ("seld_logmel_f32", "seld_logmel_i16"):
        getattr(lib, name).argtypes = [_ptr, _i64, _i64, _i64, _ptr, _int, _ptr]
    for name in ("seld_logmel_f32_strided", "seld_logmel_i16_strided"):
        getattr(lib, name).argtypes = [_ptr, _i64, _i64, _i64, _ptr, _i64, _i64, _i64, _i64, _ptr]
    for name in ("seld_stft_f32", "seld_stft_i16"):
        getattr(lib, name).argtypes = [_ptr, _i64, _i64, _i64, _ptr, _ptr]
    lib.seld_foa_intensity.argtypes = [_ptr, _i64, _i64, _ptr, _i64, _i64, _i64, _i64, _ptr]
    for fn in (lib.seld_logmel_iv_f32, lib.seld_logmel_iv_i16):
        fn.argtypes = [_ptr, _i64, _i64, _ptr, _i64, _i64, _i64, _i64, _ptr]
    for fn in (lib.seld_logmel_spectrum_f32, lib.seld_logmel_spectrum_i16):
        fn.argtypes = [_ptr, _i64, _i64, _i64, _ptr, _i64, _i64, _i64, _i64, _ptr, _ptr]
        fn.restype = ctypes.c_int
    for fn in (lib.seld_logmel_phasors_f32, lib.seld_logmel_phasors_i16):
        fn.argtypes = [_ptr, _i64, _i64, _i64, _ptr, _i64, _i64, _i64, _i64, _ptr, _ptr]
    lib.seld_phasor_pitch.restype = ctypes.c_int64
    lib.seld_phasor_pitch.argtypes = []
    lib.seld_gcc_phat_q15.argtypes = [_ptr, _i64, _i64, _i64, _ptr, _i64, _i64, _i64, _i64, _ptr]
    lib.seld_gcc_table_host.argtypes = [_ptr]
    lib.seld_gcc_phat.argtypes = [_ptr, _i64, _i64, _i64, _ptr, _i64, _i64, _i64, _i64, _ptr]
    lib.seld_nipd_table_host.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double, _ptr, _ptr, _ptr, _ptr]
    lib.seld_nipd_table_bytes.restype = _i64
    lib.seld_nipd_table_bytes.argtypes = []
    lib.seld_nipd_q15.argtypes = [_ptr, _i64, _i64, _i64, _ptr, _ptr, _i64, _i64, _i64, _i64, _ptr]
    lib.seld_labels_rasterise.argtypes = [_ptr, _i64, _i64, _int, _int, _ptr, _ptr]
    lib.seld_labels_expand.argtypes = [_ptr, _i64, _int, _ptr, _ptr]
    lib.seld_labels_rasterise_box.argtypes = [_ptr, _ptr, _i64, _i64, _int, _int, ctypes.c_double, ctypes.c_double, _ptr,
                                              _ptr]
    lib.seld_window_gather.argtypes = [_ptr, _i64, _i64, _ptr, _i64, _i64, _ptr, _ptr]
    lib.seld_window_gather_augment.argtypes = [_ptr, _i64, _int, _int, _ptr, _ptr, _i64, _i64, _ptr, ctypes.c_float, _ptr, _ptr]
    lib.seld_window_permute_mask.argtypes = [_ptr, _i64, _int, _int, _ptr, _ptr, _i64, _i64, _ptr, _ptr]
    lib.seld_foa_rotation_terms.argtypes = [_ptr, _i64, _i64, _int, _int, _ptr, _i64, _i64, _i64, _i64, _ptr]
    lib.seld_window_gather_rotate.argtypes = [_ptr, _ptr, _i64, _int, _int, _int, _int, _int, _int, _ptr, _ptr, _i64, _i64, _ptr,
                                              ctypes.c_float, _ptr, _ptr]
    lib.seld_window_permute_mask_rotate.argtypes = [_ptr, _i64, _int, _int, _ptr, _ptr, _i64, _i64, _ptr, _ptr]
    lib.seld_feature_moments_workspace.restype = _i64
    lib.seld_feature_moments_workspace.argtypes = [_i64, _int]
    lib.seld_feature_moments.argtypes = [_ptr, _i64, _int, _ptr, _ptr, _i64, _ptr]
    lib.seld_window_gather_affine.argtypes = [_ptr, _i64, _int, _ptr, _i64, _i64, _ptr, _ptr, _ptr, _ptr]
    lib.seld_window_gather_augment_affine.argtypes = [_ptr, _i64, _int, _int, _ptr, _ptr, _i64, _i64, _ptr, ctypes.c_float,
                                                      _ptr, _ptr, _ptr, _ptr]
    lib.seld_window_gather_rotate_affine.argtypes = [_ptr, _ptr, _i64, _int, _int, _int, _int, _int, _int, _ptr, _ptr, _i64,
                                                     _i64, _ptr, ctypes.c_float, _ptr, _ptr, _ptr, _ptr]
    lib.seld_window_gather_mix.argtypes = [_ptr, _i64, _int, _int, _ptr, _ptr, _ptr, _i64, _i64, _ptr, ctypes.c_float, _int,
                                           _ptr, _ptr]
    lib.seld_window_gather_mix_standardised.argtypes = [_ptr, _i64, _int, _int, _ptr, _ptr, _ptr, _i64, _i64, _ptr, ctypes.c_float,
                                                  _int, _ptr, _ptr, _ptr, _ptr]
    lib.seld_window_mix_mask.argtypes = [_ptr, _i64, _int, _int, _ptr, _ptr, _ptr, _i64, _i64, _ptr, _ptr]
    lib.seld_window_gather_mic.argtypes = [_ptr, _i64, _int, _int, _int, _ptr, _ptr, _i64, _i64, _ptr, ctypes.c_float, _ptr,
                                           _ptr]
    lib.seld_window_gather_mic_standardised.argtypes = [_ptr, _i64, _int, _int, _int, _ptr, _ptr, _i64, _i64, _ptr, ctypes.c_float,
                                                  _ptr, _ptr, _ptr, _ptr]
    lib.seld_window_spectral.argtypes = [_ptr, _i64, _int, _int, _int, _ptr, _ptr, _ptr, _ptr, _i64, _i64, ctypes.c_float, _ptr]
    lib.seld_window_spectral_standardised.argtypes = [_ptr, _i64, _int, _int, _int, _ptr, _ptr, _ptr, _ptr, _i64, _i64,
                                                      ctypes.c_float, _ptr, _ptr, _ptr]
    lib.seld_softmax_mse_workspace_bytes.restype = _i64
    lib.seld_softmax_mse_workspace_bytes.argtypes = []
    lib.seld_softmax_mse.argtypes = [_ptr, _int, _ptr, _ptr, _i64, _int, ctypes.c_float, _ptr, _ptr, _ptr, _ptr]
    lib.seld_softmax_ce_workspace_bytes.restype = _i64
    lib.seld_softmax_ce_workspace_bytes.argtypes = []
    lib.seld_softmax_ce.argtypes = [_ptr, _int, _ptr, _ptr, _i64, _int, _ptr, ctypes.c_float, ctypes.c_float, _ptr, _ptr,
                                    _ptr, _ptr]
    lib.seld_scale_by_device_scalar.argtypes = [_ptr, _int, _i64, _ptr, _ptr]
    lib.seld_smr_loss_workspace_bytes.restype = _i64
    lib.seld_smr_loss_workspace_bytes.argtypes = [_i64, _i64]
    lib.seld_smr_loss.argtypes = [_ptr, _int, _ptr, _ptr, _i64, _int, _int, _int, ctypes.c_float, ctypes.c_float,
                                  ctypes.c_float, _ptr, _ptr, _ptr, _ptr]
    lib.seld_multi_cast.argtypes = [_ptr, _ptr, _ptr, _int, _int, _ptr]
    lib.seld_stream_delay.argtypes = [_i64, _ptr]
    lib.seld_gru_fold_bias.argtypes = [_ptr, _ptr, _i64, _ptr, _int, _ptr, _ptr]
    lib.seld_gru_prepare.argtypes = [_ptr, _ptr, _ptr, _int, _i64, _ptr, _int, _ptr, _ptr, _ptr]
    lib.seld_gru_bias_grads.argtypes = [_ptr, _i64, _i64, _ptr, _ptr, _ptr]
    lib.seld_sum_chunks.argtypes = [_ptr, _int, _i64, _i64, _ptr, _int, _ptr]
    lib.seld_sum_chunks_columns.argtypes = [_ptr, _int, _i64, _i64, _i64, _i64, _ptr, _int, _ptr]
    lib.seld_gru_dwhh_finish.argtypes = [_ptr, _ptr, _int, _i64, _i64, _ptr, _int, _ptr]
    lib.seld_column_sums.argtypes = [_ptr, _int, _i64, _i64, _ptr, _ptr, _int, _ptr]
    _pp, _pi64, _pi32 = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    _f = ctypes.c_float
    _d = ctypes.c_double          # the betas: 1 - beta and 1 - beta^step are formed in double (csrc/adam.hip)
    lib.seld_multi_adam.argtypes = [_pp, _pi32, _pp, _pp, _pp, _pp, _pi64, _int, _ptr, _ptr, _d, _d, _f, _f, _f, _ptr]
    lib.seld_multi_grad_norm_scratch.argtypes = [_pi64, _int, _pi64]
    lib.seld_multi_grad_norm.argtypes = [_pp, _pi32, _pi64, _int, _f, _f, _int, _ptr, _i64, _ptr, _ptr]
    lib.seld_multi_adam_guarded.argtypes = [_pp, _pi32, _pp, _pp, _pp, _pp, _pi64, _int, _ptr, _ptr, _d, _d, _f, _f, _f, _pp, _f,
                                            _ptr, _ptr]
    lib.seld_multi_sum_chunks.argtypes = [_pp, _pp, _pi64, _pi32, _pi32, _int, _ptr]
    lib.seld_multi_column_sums_scratch.argtypes = [_pi64, _pi64, _int, _pi64]
    lib.seld_multi_column_sums.argtypes = [_pp, _pp, _pi64, _pi64, _pi32, _int, _ptr, _i64, _ptr]
    lib.seld_column_sums_blocks.argtypes = [_i64, _i64]
    lib.seld_column_sums_blocks.restype = ctypes.c_int64
    lib.seld_conv_weight_flip_transpose.argtypes = [_ptr, _int, _i64, _i64, _ptr, _ptr]
    lib.seld_conv3x3_wgrad_supported.argtypes = [_i64, _i64, _i64]
    lib.seld_conv3x3_wgrad_workspace_floats.restype = _i64
    lib.seld_conv3x3_wgrad_workspace_floats.argtypes = [_i64, _i64, _i64, _i64, _i64]
    lib.seld_conv3x3_wgrad.argtypes = [_ptr, _ptr, _i64, _i64, _i64, _i64, _i64, _ptr, _int, _ptr, _ptr]
    lib.seld_conv3x3_dgrad_supported.argtypes = [_i64, _i64, _i64]
    lib.seld_conv3x3_dgrad.argtypes = [_ptr, _ptr, _i64, _i64, _i64, _i64, _i64, _ptr, _ptr]
    lib.seld_conv3x3_forward_supported.argtypes = [_i64, _i64, _i64]
    lib.seld_conv3x3_forward_chunks.restype = _i64
    lib.seld_conv3x3_forward_chunks.argtypes = [_i64, _i64, _i64]
    lib.seld_conv3x3_forward.argtypes = [_ptr, _ptr, _i64, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr]
    lib.seld_conv_tail_partial_rows.restype = _i64
    lib.seld_conv_tail_partial_rows.argtypes = []
    lib.seld_conv_tail_forward_from_partials.argtypes = [_ptr, _int, _i64, _int, _int, _ptr, _i64, _ptr, _ptr, _ptr, _ptr,
                                                         ctypes.c_float, ctypes.c_float, _ptr, _ptr, _ptr, _ptr]
    lib.seld_convfirst_supported.argtypes = [_i64, _i64, _i64]
    lib.seld_convfirst_workspace_floats.restype = _i64
    lib.seld_convfirst_workspace_floats.argtypes = [_int]
    lib.seld_convfirst_forward.argtypes = [_ptr, _ptr, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr,
                                           ctypes.c_float, ctypes.c_float, _ptr, _ptr, _ptr, _ptr, _int, _ptr]
    lib.seld_convfirst_backward.argtypes = [_ptr, _ptr, _int, _i64, _i64, _i64, _i64, _ptr, _i64, _i64, _i64, _ptr, _ptr,
                                            _ptr, _int, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr, _int, _ptr]
    lib.seld_layernorm_supported.argtypes = [_i64]
    lib.seld_layernorm_workspace_floats.restype = _i64
    lib.seld_layernorm_workspace_floats.argtypes = [_i64, _i64]
    lib.seld_layernorm_forward.argtypes = [_ptr, _int, _i64, _i64, _ptr, _ptr, ctypes.c_float, _int, _ptr, _ptr, _ptr]
    lib.seld_layernorm_backward.argtypes = [_ptr, _ptr, _int, _i64, _i64, _ptr, _ptr, _ptr, _int, _ptr, _ptr, _ptr,
                                            _ptr, _ptr]
    lib.seld_conv_tail_workspace_floats.restype = _i64
    lib.seld_conv_tail_workspace_floats.argtypes = [_int]
    lib.seld_conv_tail_forward.argtypes = [_ptr, _ptr, _int, _i64, _int, _int, _ptr, _ptr, _ptr, _ptr, ctypes.c_float,
                                           ctypes.c_float, _int, _ptr, _ptr, _ptr, _ptr, _ptr]
    lib.seld_conv_tail_backward.argtypes = [_ptr, _ptr, _ptr, _int, _i64, _int, _int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                            _ptr, _ptr]
    lib.seld_dwconv1d.argtypes = [_ptr, _int, _ptr, _ptr, _i64, _i64, _int, _int, _int, _ptr, _ptr]
    lib.seld_dwconv1d_wgrad.argtypes = [_ptr, _ptr, _int, _i64, _i64, _int, _int, _ptr, _ptr]
    lib.seld_dwconv1d_wgrad_rows.argtypes = [_i64, _i64]
    lib.seld_dwconv1d_wgrad_rows.restype = ctypes.c_int64
    lib.seld_gru_to_tile.argtypes = [_ptr, _int, _i64, _i64, _int, _ptr, _ptr]
    lib.seld_gru_from_pair_tile.argtypes = [_ptr, _int, _i64, _i64, _ptr, _ptr, _ptr]
    lib.seld_gru_previous_state.argtypes = [_ptr, _int, _i64, _i64, _ptr, _ptr]
    lib.seld_gru_tile_rows.restype = _i64
    lib.seld_gru_tile_rows.argtypes = []
    lib.seld_gru_forward.argtypes = [_ptr, _int, _ptr, _ptr, _i64, _i64, _i64, _ptr, _ptr, _ptr]
    lib.seld_gru_backward.argtypes = [_ptr, _ptr, _ptr, _int, _ptr, _i64, _i64, _i64, _ptr, _ptr, _ptr]
    lib.seld_gru_backward_direct.argtypes = [_ptr, _ptr, _ptr, _int, _ptr, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr]
    lib.seld_grid_decode.argtypes = [_ptr, _int, _i64, _i64, _i64, _i64, _ptr, _ptr, _i64, _i64, ctypes.c_float, _int,
                                     _ptr, _ptr, _ptr, _ptr, _ptr]
    lib.seld_doa_match.argtypes = [_ptr, _ptr, _int, _ptr, _ptr, _i64, _int, _int, ctypes.c_double, _ptr, _ptr, _ptr]
    lib.seld_grid_decode_tta.argtypes = [_ptr, _int, _i64, _i64, _i64, _i64, _ptr, _ptr, _i64, _i64, _pi32, _int,
                                         ctypes.c_float, _int, _ptr, _ptr, _ptr, _ptr, _ptr]
    lib.seld_track_link.argtypes = [_ptr, _ptr, _int, _ptr, _i64, _ptr, _int, _int, _int, _int, _int, _ptr, _ptr, _ptr, _ptr,
                                    _ptr, _ptr, _ptr]
    lib.seld_grid_decode_refine.argtypes = [_ptr, _int, _i64, _i64, _i64, _i64, _ptr, _ptr, _i64, _i64, _pi32, _int,
                                            ctypes.c_float, _int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]
    lib.seld_doa_match_dirs.argtypes = [_ptr, _ptr, _int, _ptr, _ptr, _i64, ctypes.c_double, _ptr, _ptr, _ptr]
    lib.seld_doa_match_prefix.argtypes = [_ptr, _ptr, _ptr, _int, _ptr, _ptr, _i64, _int, _int, ctypes.c_double, _ptr, _ptr,
                                          _ptr]
    lib.seld_sweep_score.argtypes = [_ptr, _ptr, _ptr, _ptr, _int, _ptr, _i64, ctypes.POINTER(ctypes.c_float), _int, _i64,
                                     _ptr, _ptr, _ptr, _ptr]
    lib.seld_doa_assign.argtypes = [_ptr, _ptr, _ptr, _int, _ptr, _ptr, _i64, _int, _int, ctypes.c_double, _ptr, _ptr]
    lib.seld_segment_score.argtypes = [_ptr, _ptr, _int, _ptr, _ptr, _ptr, _i64, ctypes.c_double, _ptr, _ptr, _ptr, _ptr,
                                       _ptr, _ptr]
    lib.seld_jackknife_score.argtypes = [_ptr, _ptr, _ptr, _i64, _ptr, _ptr, _ptr]
    lib.seld_resample_plan.argtypes =[_i64, _i64, _pi32, _pi32, _pi32, _pi32]
    lib.seld_resample_table_host.argtypes = [_i64, _i64, _ptr, _ptr]
    for fn in (lib.seld_resample_f32, lib.seld_resample_i16):
        fn.argtypes = [_ptr, _i64, _i64, _i64, _ptr, _int, _int, _int, _int, _ptr, _i64, _ptr]
    lib.seld_frame_class_mask.argtypes = [_ptr, _i64, _int, _ptr, _ptr]
    lib.seld_window_class_frames.argtypes = [_ptr, _i64, _i64, _i64, _i64, _int, _ptr, _ptr]
    lib.seld_pcen_workspace.restype = _i64
    lib.seld_pcen_workspace.argtypes = [_i64, _i64, _int, _int]
    lib.seld_pcen.argtypes = [_ptr, _ptr, _i64, _i64, _int, _int, _f, _f, _f, _f, _f, _ptr, _i64, _ptr]
    return lib


def load_library():
    """Load (once) and return the ctypes handle.  Fails loudly when the .so is absent."""
    global _lib
    if _lib is not None:                     # hot path: ~40 calls per optimiser iteration on an enqueue-bound step
        return _lib
    with _lock:
        if _lib is None:
            if not LIB_PATH.exists():
                raise SeldNativeError(
                    f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    f"or `make -C {_HERE / 'csrc'}`.  There is no CPU fallback.")
            lib = _declare(ctypes.CDLL(str(LIB_PATH)))
            global GRU_TILE
            GRU_TILE = int(lib.seld_gru_tile_rows())       # geometry of THIS build, before anything sizes a buffer
            _lib = lib
        return _lib


def check(rc: int, what: str = "libseld_hip"):
    if rc != 0:
        msg = load_library().seld_last_error()
        raise SeldNativeError(f"{what} failed with code {rc}: {msg.decode() if msg else '?'}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_ptr(device) -> ctypes.c_void_p:
    """The caller's current stream on ``device`` as a hipStream_t.  The raw accessor skips the Stream wrapper object
    (~5 us per call; two dozen launches per iteration take their stream here)."""
    if _raw_stream is not None:
        index = device.index if isinstance(device, torch.device) else torch.device(device).index
        return ctypes.c_void_p(_raw_stream(index if index is not None else torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def mel_filterbank() -> torch.Tensor:
    """fp32 HTK filterbank [481, 64] built with the same torch ops as
    ``torchaudio.functional.melscale_fbanks(481, 0, 12000, 64, 24000, norm=None, mel_scale='htk')``
    (the constant inside the MelScale the reference instantiates at dataset.py:38-43)."""
    import math
    all_freqs = torch.linspace(0, 24000 // 2, N_BINS)
    m_max = 2595.0 * math.log10(1.0 + 12000.0 / 700.0)
    m_pts = torch.linspace(0.0, m_max, N_MELS + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    rising = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    falling = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.min(rising, falling), min=0.0).contiguous()


def ensure_init(device) -> int:
    """seld_init for ``device`` (idempotent) and upload of the torch-built mel table."""
    if isinstance(device, torch.device) and device.index in _initialised_devices:     # hot path, no lock
        return device.index
    device = torch.device(device)
    if device.type != "cuda":
        raise SeldNativeError(f"the SELD HIP path needs a ROCm device, got {device}")
    index = device.index if device.index is not None else torch.cuda.current_device()
    lib = load_library()
    with _lock:
        if index in _initialised_devices:
            return index
    with _device_guard(index):
        check(lib.seld_init(index), "seld_init")
        fb = mel_filterbank()
        check(lib.seld_set_mel_filterbank(ctypes.c_void_p(fb.data_ptr())), "seld_set_mel_filterbank")
        win = torch.hann_window(N_FFT, periodic=True, dtype=torch.float32).contiguous()
        check(lib.seld_set_window(ctypes.c_void_p(win.data_ptr())), "seld_set_window")
    with _lock:
        _initialised_devices.add(index)
    return index


def num_cus(device=None) -> int:
    """The compute-unit count the library sizes its grids, workspaces and plans from on ``device`` (default: the current
    one): the device's own, or the lower one the developer switch SELD_CUS set when seld_init ran."""
    index = ensure_init(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
    with _device_guard(index):
        n = int(load_library().seld_num_cus())
    if n < 1:
        check(n, "seld_num_cus")
    return n


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _device_guard(index: int):
    """``torch.cuda.device(index)`` only when a switch is needed: one process drives one GPU (one rank per GPU), so
    the current device is almost always right and the context manager's two runtime calls (~15 us of host time per
    kernel launch on a launch-bound model) are skipped."""
    return _NO_GUARD if torch.cuda.current_device() == index else torch.cuda.device(index)


def num_frames(num_samples: int) -> int:
    return 1 + int(num_samples) // HOP


def logmel(pcm: torch.Tensor, layout: str = "cft", out: torch.Tensor | None = None) -> torch.Tensor:
    """Fused log-mel on the GPU.  ``pcm``: [N, C, L] or [C, L], float32 in [-1, 1) or int16.

    layout 'cft' -> [N, C, 64, F] (reference layout, dataset.py:53)
    layout 'tcf' -> [N, F, C, 64] (time-major; windows are contiguous slices)
    """
    squeeze = pcm.dim() == 2
    if squeeze:
        pcm = pcm.unsqueeze(0)
    if pcm.dim() != 3:
        raise ValueError("pcm must be [N, C, L] or [C, L]")
    if not pcm.is_cuda:
        raise SeldNativeError("logmel: pcm must live on the GPU (no CPU fallback in the product path)")
    if pcm.dtype not in (torch.float32, torch.int16):
        raise TypeError(f"logmel: pcm dtype must be float32 or int16, got {pcm.dtype}")
    pcm = pcm.contiguous()
    n, c, length = pcm.shape
    index = ensure_init(pcm.device)
    frames = num_frames(length)
    code = {"cft": 0, "tcf": 1}[layout]
    shape = (n, c, N_MELS, frames) if code == 0 else (n, frames, c, N_MELS)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=pcm.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"logmel: out must be contiguous float32 {shape}")
    lib = load_library()
    fn = lib.seld_logmel_f32 if pcm.dtype == torch.float32 else lib.seld_logmel_i16
    with _device_guard(index):
        check(fn(ctypes.c_void_p(pcm.data_ptr()), n, c, length, ctypes.c_void_p(out.data_ptr()), code,
                 _stream_ptr(pcm.device)), "seld_logmel")
    return out[0] if squeeze else out


# --------------------------------------------------------------------------- sample-rate conversion

SAMPLE_RATE = 24000
_resample_tables = {}


def resample_plan(rate_in: int, rate_out: int = SAMPLE_RATE):
    """(up, down, taps, half) of the designed polyphase table for ``rate_in -> rate_out``; host
    only.  Raises for a rate the design does not cover (more than 320 phases or 1100 taps per output)."""
    vals = [ctypes.c_int32() for _ in range(4)]
    check(load_library().seld_resample_plan(int(rate_in), int(rate_out), *[ctypes.byref(v) for v in vals]),
          "seld_resample_plan")
    return tuple(int(v.value) for v in vals)


def resample_length(num_samples: int, rate_in: int, rate_out: int = SAMPLE_RATE) -> int:
    """Output samples for ``num_samples`` input samples: ceil(L * up / down), exact integers."""
    up, down, _, _ = resample_plan(rate_in, rate_out)
    return -((-int(num_samples) * up) // down)


def resample_table(rate_in: int, rate_out: int = SAMPLE_RATE):
    """The designed table on the host: (float32 [up, taps], float64 [up, taps]) as numpy arrays."""
    import numpy as np
    up, _, taps, _ = resample_plan(rate_in, rate_out)
    t32, t64 = np.zeros((up, taps), dtype=np.float32), np.zeros((up, taps), dtype=np.float64)
    check(load_library().seld_resample_table_host(int(rate_in), int(rate_out), ctypes.c_void_p(t32.ctypes.data),
                                                  ctypes.c_void_p(t64.ctypes.data)), "seld_resample_table_host")
    return t32, t64


def _resample_table_device(rate_in: int, rate_out: int, device, index: int):
    """The table of a rate pair, designed once and kept on the device it was asked for."""
    key = (int(rate_in), int(rate_out), index)
    hit = _resample_tables.get(key)
    if hit is None:
        plan = resample_plan(rate_in, rate_out)
        hit = (plan, torch.from_numpy(resample_table(rate_in, rate_out)[0]).to(device))
        _resample_tables[key] = hit
    return hit


def resample(pcm: torch.Tensor, rate_in: int, rate_out: int = SAMPLE_RATE, out: torch.Tensor | None = None) -> torch.Tensor:
    """Sample-rate conversion on the GPU (csrc/resample.hip).  ``pcm``: [N, C, L] or [C, L], float32 in [-1, 1) or int16
    (scaled by 2^-15), contiguous; returns float32 [N, C, ceil(L * up / down)] (or [C, ...]): what the 24 kHz feature
    kernels take as it is.  The table of a rate pair is designed on first use and stays on the device."""
    squeeze = pcm.dim() == 2
    if squeeze:
        pcm = pcm.unsqueeze(0)
    if pcm.dim() != 3:
        raise ValueError("pcm must be [N, C, L] or [C, L]")
    if not pcm.is_cuda:
        raise SeldNativeError("resample: pcm must live on the GPU (no CPU fallback in the product path)")
    if pcm.dtype not in (torch.float32, torch.int16):
        raise TypeError(f"resample: pcm dtype must be float32 or int16, got {pcm.dtype}")
    if not pcm.is_contiguous():
        raise ValueError("resample: pcm must be contiguous")
    n, c, length = pcm.shape
    index = ensure_init(pcm.device)
    (up, down, taps, half), table = _resample_table_device(rate_in, rate_out, pcm.device, index)
    out_len = -((-length * up) // down)
    shape = (n, c, out_len)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=pcm.device)
    else:
        if squeeze and out.dim() == 2:                      # [C, L] in: [C, L_out] out
            out = out.unsqueeze(0)
        if tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != pcm.device:
            raise ValueError(f"resample: out must be contiguous float32 {shape[1:] if squeeze else shape} on {pcm.device}")
    lib = load_library()
    fn = lib.seld_resample_f32 if pcm.dtype == torch.float32 else lib.seld_resample_i16
    with _device_guard(index):
        check(fn(ctypes.c_void_p(pcm.data_ptr()), n, c, length, ctypes.c_void_p(table.data_ptr()), up, down, taps, half,
                 ctypes.c_void_p(out.data_ptr()), out_len, _stream_ptr(pcm.device)), "seld_resample")
    return out[0] if squeeze else out


# --------------------------------------------------------------------------- labels / windows

GRID_I, GRID_J = 18, 36
NUM_CLASSES = 14


def _p(t: torch.Tensor | None):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def rasterise_labels(events: torch.Tensor, total_frames: int, I: int = GRID_I, J: int = GRID_J,
                     device=None, out: torch.Tensor | None = None) -> torch.Tensor:
    """dataset.py:60-119 on the GPU.  ``events``: int [R, 5] rows (meta_frame, class, source, az, el).
    Returns the compact class mask, uint16 [total_frames, I*J] (bit c <=> class c active)."""
    events = torch.as_tensor(events)
    if events.numel() and (events.dim() != 2 or events.shape[1] < 5):
        raise ValueError("events must be [R, >=5]")
    if events.numel() and not events.is_cuda:      # host rows are validated; device rows are trusted (no sync)
        cls = events[:, 1]
        if int(cls.max()) >= NUM_CLASSES or int(cls.min()) < 0:
            raise IndexError("metadata class index out of range for 14 classes (dataset.py:110)")
    device = torch.device(device) if device is not None else (events.device if events.is_cuda else None)
    if device is None:
        raise SeldNativeError("rasterise_labels: pass device= (no CPU fallback)")
    index = ensure_init(device)
    ev = events[:, :5].to(device=device, dtype=torch.int32).contiguous() if events.numel() else \
        torch.zeros((0, 5), dtype=torch.int32, device=device)
    if out is None:
        out = torch.empty((total_frames, I * J), dtype=torch.uint16, device=device)
    elif tuple(out.shape) != (total_frames, I * J) or out.dtype != torch.uint16 or not out.is_contiguous():
        raise ValueError("rasterise_labels: out must be a contiguous uint16 [total_frames, I*J] tensor")
    with _device_guard(index):
        check(load_library().seld_labels_rasterise(_p(ev), ev.shape[0], total_frames, I, J, _p(out),
                                                   _stream_ptr(device)), "seld_labels_rasterise")
    return out


def gaussian_source_noise(events, sigma_az: float = 5.0, sigma_el: float = 5.0, rng=None):
    """One (azimuth, elevation) normal draw per unique (class, source) pair, in the sorted-key order of
    ``df.groupby([1, 2])`` (smrl_seld_gaussian.py:426-437).  Returns float64 [R, 2]: the box centre of every row.
    ``rng``: a numpy Generator / RandomState; default ``numpy.random`` (the reference never seeds)."""
    import numpy as np
    ev = np.asarray(events)[:, :5].astype(np.int64)
    rng = np.random if rng is None else rng
    keys = sorted({(int(c), int(s)) for c, s in ev[:, 1:3]})
    noise = {k: (rng.normal(0, sigma_az), rng.normal(0, sigma_el)) for k in keys}
    centres = np.empty((ev.shape[0], 2), dtype=np.float64)
    for r, row in enumerate(ev):
        dn = noise[(int(row[1]), int(row[2]))]
        centres[r] = (row[3] + dn[0], row[4] + dn[1])
    return centres


def rasterise_labels_gaussian(events, centres, total_frames: int, I: int = GRID_I, J: int = GRID_J,
                              sigma_az: float = 5.0, sigma_el: float = 5.0, device=None) -> torch.Tensor:
    """smrl_seld_gaussian.py:397-534 on the GPU: uint16 class mask [total_frames, I*J]."""
    events = torch.as_tensor(events)
    if events.numel() and not events.is_cuda:
        cls = events[:, 1]
        if int(cls.max()) >= NUM_CLASSES or int(cls.min()) < 0:
            raise IndexError("metadata class index out of range for 14 classes")
    device = torch.device(device) if device is not None else (events.device if events.is_cuda else None)
    if device is None:
        raise SeldNativeError("rasterise_labels_gaussian: pass device= (no CPU fallback)")
    index = ensure_init(device)
    ev = events[:, :5].to(device=device, dtype=torch.int32).contiguous() if events.numel() else \
        torch.zeros((0, 5), dtype=torch.int32, device=device)
    ctr = torch.as_tensor(centres, dtype=torch.float64).to(device).contiguous().reshape(-1, 2)
    if ctr.shape[0] != ev.shape[0]:
        raise ValueError("one box centre per metadata row")
    out = torch.empty((total_frames, I * J), dtype=torch.uint16, device=device)
    with _device_guard(index):
        check(load_library().seld_labels_rasterise_box(_p(ev), _p(ctr), ev.shape[0], total_frames, I, J, float(sigma_az),
                                                       float(sigma_el), _p(out), _stream_ptr(device)),
              "seld_labels_rasterise_box")
    return out


def expand_labels(mask: torch.Tensor, num_classes: int = NUM_CLASSES) -> torch.Tensor:
    """uint16 [..., G] -> float32 [..., G, num_classes] (dataset.py:110-117 semantics)."""
    if not mask.is_cuda or mask.dtype != torch.uint16:
        raise SeldNativeError("expand_labels: mask must be a uint16 GPU tensor")
    mask = mask.contiguous()
    index = ensure_init(mask.device)
    out = torch.empty(tuple(mask.shape) + (num_classes,), dtype=torch.float32, device=mask.device)
    with _device_guard(index):
        check(load_library().seld_labels_expand(_p(mask), mask.numel(), num_classes, _p(out),
                                                _stream_ptr(mask.device)), "seld_labels_expand")
    return out


def _window_call(name: str, src: torch.Tensor, dtype, row, what: str, starts: torch.Tensor, window: int,
                 params: torch.Tensor | None, out: torch.Tensor | None):
    """The front of the five window gathers, every message opening with ``name``: the source (on the GPU; ``dtype`` unless
    None; rows of shape ``row`` unless None, a None extent being free; at least one row -- ``what`` words the refusal),
    ``starts`` as int64 on the source's device, ``params`` (None: the gather takes none) a contiguous int32 [B, 12] tensor
    there, ``out`` allocated or checked as [B, window] + the row shape.  Returns (src, device index, starts, out)."""
    ok = src.is_cuda and (dtype is None or src.dtype == dtype)
    if ok and row is not None:
        ok = src.dim() == len(row) + 1 and all(r is None or n == r for n, r in zip(src.shape[1:], row))
    if not ok:
        raise SeldNativeError(f"{name}: src must be {what}")
    src = src.contiguous()
    if src.shape[0] == 0:
        raise ValueError(f"{name}: empty source")
    index = ensure_init(src.device)
    starts = starts.to(device=src.device, dtype=torch.int64).contiguous()
    if params is not None and (not params.is_cuda or params.dtype != torch.int32 or not params.is_contiguous()
                               or tuple(params.shape) != (starts.numel(), AUGMENT_PARAM_INTS)):
        raise ValueError(f"{name}: params must be a contiguous int32 [B, 12] GPU tensor (augment_params)")
    shape = (starts.numel(), window) + tuple(src.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=src.dtype, device=src.device)
    elif tuple(out.shape) != shape or out.dtype != src.dtype or out.device != src.device or not out.is_contiguous():
        kind = str(src.dtype).replace("torch.", "")
        raise ValueError(f"{name}: out must be a contiguous {kind} tensor of shape {shape} on {src.device}")
    return src, index, starts, out


def _channel_table(name: str, channel_table, channels: int):
    """The host's uint8 [16, channels] channel table as a contiguous numpy array."""
    import numpy as np
    table = np.ascontiguousarray(channel_table, dtype=np.uint8)
    if table.shape != (AUGMENT_PATTERNS, channels):
        raise ValueError(f"{name}: channel_table must be [16, {channels}]")
    return table


def gather_windows(src: torch.Tensor, starts: torch.Tensor, window: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """dataset.py:267-317: src [T, ...] (time-major rows) -> [B, window, ...], zero padded past T.  ``out``: write into
    this contiguous tensor of that shape (the static input buffer of a captured training step)."""
    src, index, starts, out = _window_call("gather_windows", src, None, None, "a GPU tensor", starts, window, None, out)
    row_bytes = src[0].numel() * src.element_size()
    if row_bytes == 0:
        raise ValueError("gather_windows: empty source")
    with _device_guard(index):
        check(load_library().seld_window_gather(_p(src), src.shape[0], row_bytes, _p(starts), starts.numel(),
                                                window, _p(out), _stream_ptr(src.device)), "seld_window_gather")
    return out


def _affine_tables(name: str, scale, shift, src: torch.Tensor):
    """The [C, 64] float32 scale / shift tables of the standardising gathers on ``src``'s device, or
    (None, None) when neither is given; one without the other is refused."""
    if scale is None and shift is None:
        return None, None
    if scale is None or shift is None:
        raise ValueError(f"{name}: scale and shift come together")
    shape = (int(src.shape[1]), N_MELS)
    for what, t in (("scale", scale), ("shift", shift)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == src.device and t.dtype == torch.float32
                and tuple(t.shape) == shape):
            raise SeldNativeError(f"{name}: {what} must be a float32 tensor {list(shape)} on {src.device}")
    return scale.contiguous(), shift.contiguous()


def gather_windows_affine(src: torch.Tensor, starts: torch.Tensor, window: int, scale: torch.Tensor, shift: torch.Tensor,
                          out: torch.Tensor | None = None) -> torch.Tensor:
    """``gather_windows`` of the feature timeline src [T, C, 64] (float32) with every element inside the timeline mapped to
    ``fmaf(x, scale[c, f], shift[c, f])`` on the way (csrc/labels.hip, the standardising instantiation of the plain gather);
    rows past the timeline stay zero.  ``scale`` / ``shift``: float32 [C, 64] on the device."""
    src, index, starts, out = _window_call("gather_windows_affine", src, torch.float32, (None, N_MELS),
                                           "a float32 GPU tensor [T, C, 64]", starts, window, None, out)
    if src.shape[1] == 0:
        raise ValueError("gather_windows_affine: empty source")
    if scale is None or shift is None:
        raise ValueError("gather_windows_affine: scale and shift are required")
    scale, shift = _affine_tables("gather_windows_affine", scale, shift, src)
    with _device_guard(index):
        check(load_library().seld_window_gather_affine(_p(src), src.shape[0], int(src.shape[1]), _p(starts), starts.numel(),
                                                       window, _p(scale), _p(shift), _p(out), _stream_ptr(src.device)),
              "seld_window_gather_affine")
    return out


def feature_moments(spec_tm: torch.Tensor) -> torch.Tensor:
    """Moments of a time-major feature timeline spec_tm [T, C, 64] (float32, on the GPU): float64 [2, C, 64] on the device,
    (sum x, sum x^2) over the frames per (channel, bin) in the fixed order of include/seld_hip.h -- the same bits on every
    device and grid (csrc/standardise.hip).  The timeline is read once; the slab partials live in a workspace from the
    caching allocator, freed on return (stream-ordered: the allocator reuses it only behind this stream's work)."""
    if not (isinstance(spec_tm, torch.Tensor) and spec_tm.is_cuda and spec_tm.dtype == torch.float32 and spec_tm.dim() == 3
            and spec_tm.shape[2] == N_MELS):
        raise SeldNativeError("feature_moments: spec_tm must be a float32 GPU tensor [T, C, 64]")
    if spec_tm.shape[0] == 0 or spec_tm.shape[1] == 0:
        raise ValueError("feature_moments: empty timeline")
    spec_tm = spec_tm.contiguous()
    index = ensure_init(spec_tm.device)
    lib = load_library()
    frames, channels = int(spec_tm.shape[0]), int(spec_tm.shape[1])
    nbytes = int(lib.seld_feature_moments_workspace(frames, channels))
    with _device_guard(index):
        workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=spec_tm.device)
        moments = torch.empty((2, channels, N_MELS), dtype=torch.float64, device=spec_tm.device)
        check(lib.seld_feature_moments(_p(spec_tm), frames, channels, _p(moments), _p(workspace), nbytes,
                                       _stream_ptr(spec_tm.device)), "seld_feature_moments")
    return moments


PCEN_CHUNK_FRAMES = 256           # SELD_PCEN_CHUNK_FRAMES
PCEN_FRAME_RATE = 50.0            # feature frames per second: hop 480 at 24 kHz


def pcen_coefficient(tau: float) -> float:
    """The smoother's coefficient s of a time constant ``tau`` in seconds at 50 frames per second, in float64:
    T_f = 50 tau, s = (sqrt(1 + 4 T_f^2) - 1) / (2 T_f^2) -- evaluated as 2 / (1 + sqrt(1 + 4 T_f^2)), the same number
    without the cancellation at small tau (tau -> 0 gives s -> 1, a smoother that follows the input)."""
    import math
    tau = float(tau)
    if not (math.isfinite(tau) and tau > 0.0):
        raise ValueError(f"pcen_coefficient: the time constant must be finite and positive, got {tau}")
    tf = PCEN_FRAME_RATE * tau
    return 2.0 / (1.0 + math.sqrt(1.0 + 4.0 * tf * tf))


def pcen(features: torch.Tensor, c_log: int, s: float, alpha: float, delta: float, r: float, eps: float,
         out: torch.Tensor | None = None) -> torch.Tensor:
    """Per-channel energy normalisation of the first ``c_log`` (log-mel, dB) channels of time-major features
    [T, C, 64] (one clip) or [N, T, C, 64] (float32, on the GPU; csrc/pcen.hip):
    y = (E (eps + M)^-alpha + delta)^r - delta^r with E the mel power behind the stored dB value and M its first-order
    average along time with coefficient ``s`` (``pcen_coefficient``), restarted in every clip.  ``out``: None (a new tensor:
    the other channels are copied from ``features``), ``features`` itself (in place) or a tensor of its shape whose other
    channels are left as they are.  The chunk carries live in a workspace from the caching allocator, freed on return
    (stream-ordered: the allocator reuses it only behind this stream's work).  Out-of-range parameters are refused by the
    library (SeldNativeError) before any launch."""
    if not (isinstance(features, torch.Tensor) and features.is_cuda and features.dtype == torch.float32
            and features.dim() in (3, 4) and features.shape[-1] == N_MELS and features.is_contiguous()):
        raise SeldNativeError("pcen: features must be a contiguous float32 GPU tensor [T, C, 64] or [N, T, C, 64]")
    if features.numel() == 0:
        raise ValueError("pcen: empty features")
    if out is None:
        out = features.clone()
    elif not (isinstance(out, torch.Tensor) and out.device == features.device and out.dtype == torch.float32
              and out.shape == features.shape and out.is_contiguous()):
        raise SeldNativeError("pcen: out must be a contiguous float32 tensor of the features' shape on their device")
    index = ensure_init(features.device)
    lib = load_library()
    clips = int(features.shape[0]) if features.dim() == 4 else 1
    frames, channels = int(features.shape[-3]), int(features.shape[-2])
    nbytes = int(lib.seld_pcen_workspace(clips, frames, channels, int(c_log)))
    with _device_guard(index):
        workspace = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=features.device)
        check(lib.seld_pcen(_p(features), _p(out), clips, frames, channels, int(c_log), float(s), float(alpha), float(delta),
                            float(r), float(eps), _p(workspace), nbytes, _stream_ptr(features.device)), "seld_pcen")
    return out


BALANCE_COLUMNS = 16             # SELD_BALANCE_COLUMNS: classes 0..13, frames with any class, frames inside the timeline
BALANCE_MAX_CLASSES = 14          # SELD_BALANCE_MAX_CLASSES


def frame_class_mask(mask_tm: torch.Tensor) -> torch.Tensor:
    """The classes active anywhere on the grid, per frame: uint16 [T] on the device, the bitwise OR over the cells of every
    row of the label timeline mask_tm [T, cells] (uint16, on the GPU, cells a multiple of 8).  The timeline is read once
    (csrc/balance.hip)."""
    if not (isinstance(mask_tm, torch.Tensor) and mask_tm.is_cuda and mask_tm.dtype == torch.uint16 and mask_tm.dim() == 2):
        raise SeldNativeError("frame_class_mask: mask_tm must be a uint16 GPU tensor [T, cells]")
    if mask_tm.shape[0] == 0 or mask_tm.shape[1] == 0:
        raise ValueError("frame_class_mask: empty timeline")
    mask_tm = mask_tm.contiguous()
    if mask_tm.shape[1] % 8 != 0 or mask_tm.shape[1] > 2048:
        raise SeldNativeError(f"frame_class_mask: cells must be a multiple of 8, at most 2048 (rows are read in 16-byte chunks), "
                              f"got {mask_tm.shape[1]}")
    if mask_tm.data_ptr() % 16 != 0:                 # the entry point wants 16-byte alignment (-4 otherwise): a view that
        mask_tm = mask_tm.clone()                    # starts off it inside its allocation is copied to a fresh one
    index = ensure_init(mask_tm.device)
    with _device_guard(index):
        out = torch.empty((mask_tm.shape[0],), dtype=torch.uint16, device=mask_tm.device)
        check(load_library().seld_frame_class_mask(_p(mask_tm), int(mask_tm.shape[0]), int(mask_tm.shape[1]), _p(out),
                                                   _stream_ptr(mask_tm.device)), "seld_frame_class_mask")
    return out


def window_class_frames(frame_mask: torch.Tensor, window: int, hop: int, n_windows: int, num_classes: int) -> torch.Tensor:
    """int32 [n_windows, 16] on the device from the per-frame class words of ``frame_class_mask``: for window w, covering
    the frames [w hop, min(w hop + window, T)), column c < num_classes = frames with class c active, column 14 = frames
    with any of them active, column 15 = frames inside the timeline (csrc/balance.hip)."""
    if not (isinstance(frame_mask, torch.Tensor) and frame_mask.is_cuda and frame_mask.dtype == torch.uint16
            and frame_mask.dim() == 1):
        raise SeldNativeError("window_class_frames: frame_mask must be a uint16 GPU tensor [T]")
    frame_mask = frame_mask.contiguous()
    index = ensure_init(frame_mask.device)
    with _device_guard(index):
        out = torch.empty((max(int(n_windows), 0), BALANCE_COLUMNS), dtype=torch.int32, device=frame_mask.device)
        check(load_library().seld_window_class_frames(_p(frame_mask), int(frame_mask.shape[0]), int(window), int(hop),
                                                      int(n_windows), int(num_classes), _p(out),
                                                      _stream_ptr(frame_mask.device)), "seld_window_class_frames")
    return out


def augment_params(params, batch: int, window: int, device, steps: int | None = None) -> torch.Tensor:
    """The per-window parameter table of the augmenting gathers as an int32 [batch, 12] device tensor.  A host table
    (numpy array / CPU tensor) is validated here -- pattern in 0..15, every mask inside its axis, and with ``steps`` (the J
    of the rotating gathers) the azimuth step [9] in 0..steps-1 -- and uploaded with one asynchronous copy; a device tensor
    is trusted (no synchronise; the kernels clamp whatever they are given)."""
    t = torch.as_tensor(params)
    if tuple(t.shape) != (batch, AUGMENT_PARAM_INTS):
        raise ValueError(f"augment parameters must be [{batch}, {AUGMENT_PARAM_INTS}], got {tuple(t.shape)}")
    if t.is_cuda:
        if t.dtype != torch.int32:
            raise TypeError("augment parameters on the device must be int32")
        return t.contiguous()
    t = t.to(torch.int32).contiguous()
    if batch:
        if int(t[:, 0].min()) < 0 or int(t[:, 0].max()) >= AUGMENT_PATTERNS:
            raise ValueError("augment parameters: spatial pattern outside 0..15")
        for first, axis, what in ((1, window, "time"), (3, window, "time"), (5, N_MELS, "frequency"), (7, N_MELS, "frequency")):
            start, length = t[:, first], t[:, first + 1]
            if int(start.min()) < 0 or int(length.min()) < 0 or int((start + length).max()) > axis:
                raise ValueError(f"augment parameters: {what} mask outside [0, {axis})")
        if steps is not None and (int(t[:, 9].min()) < 0 or int(t[:, 9].max()) >= int(steps)):
            raise ValueError(f"augment parameters: azimuth step outside 0..{int(steps) - 1}")
    return t.to(device, non_blocking=True)


def gather_windows_augment(src: torch.Tensor, starts: torch.Tensor, window: int, params: torch.Tensor, channel_table=None,
                           freq_channels: int | None = None, mask_value: float = 0.0,
                           out: torch.Tensor | None = None, scale: torch.Tensor | None = None,
                           shift: torch.Tensor | None = None) -> torch.Tensor:
    """``gather_windows`` of the feature timeline src [T, C, 64] (float32) with one augmentation per window
    (csrc/augment.hip): a signed channel permutation chosen by the window's spatial pattern, then time / frequency masks.
    ``params``: int32 [B, 12] on the device (``augment_params``); ``channel_table``: uint8 [16, C] host array, entry =
    source channel | 0x80 when negated (None: channels stay put); frequency masks touch channels < ``freq_channels``.
    ``scale`` / ``shift`` (float32 [C, 64] on the device, both or neither): the standardising export -- the copied value of
    OUTPUT channel c becomes ``fmaf(v, scale[c, f], shift[c, f])`` before the masks."""
    src, index, starts, out = _window_call("gather_windows_augment", src, torch.float32, (None, N_MELS),
                                           "a float32 GPU tensor [T, C, 64]", starts, window, params, out)
    channels = int(src.shape[1])
    freq_channels = channels if freq_channels is None else int(freq_channels)
    table = None if channel_table is None else _channel_table("gather_windows_augment", channel_table, channels)
    scale, shift = _affine_tables("gather_windows_augment", scale, shift, src)
    if scale is not None:
        with _device_guard(index):
            check(load_library().seld_window_gather_augment_affine(
                _p(src), src.shape[0], channels, freq_channels, _p(starts), _p(params), starts.numel(), window,
                ctypes.c_void_p(table.ctypes.data) if table is not None else None, float(mask_value), _p(scale), _p(shift),
                _p(out), _stream_ptr(src.device)), "seld_window_gather_augment_affine")
        return out
    with _device_guard(index):
        check(load_library().seld_window_gather_augment(
            _p(src), src.shape[0], channels, freq_channels, _p(starts), _p(params), starts.numel(), window,
            ctypes.c_void_p(table.ctypes.data) if table is not None else None, float(mask_value), _p(out),
            _stream_ptr(src.device)), "seld_window_gather_augment")
    return out


def gather_windows_permute(src: torch.Tensor, starts: torch.Tensor, window: int, params: torch.Tensor, I: int = GRID_I,
                           J: int = GRID_J, out: torch.Tensor | None = None) -> torch.Tensor:
    """``gather_windows`` of the label timeline src [T, I*J] (uint16 class masks) with the grid cells moved by each
    window's spatial pattern (csrc/augment.hip); labels are never masked."""
    src, index, starts, out = _window_call("gather_windows_permute", src, torch.uint16, (I * J,),
                                           "a uint16 GPU tensor [T, I*J]", starts, window, params, out)
    with _device_guard(index):
        check(load_library().seld_window_permute_mask(_p(src), src.shape[0], I, J, _p(starts), _p(params), starts.numel(),
                                                      window, _p(out), _stream_ptr(src.device)), "seld_window_permute_mask")
    return out


MIC_KINDS = {"logmel_gcc": 0, "logmel_nipd": 1}        # SELD_MIC_GCC, SELD_MIC_NIPD


def gather_windows_mic(src: torch.Tensor, starts: torch.Tensor, window: int, params: torch.Tensor, mic_perm, kind: str,
                       freq_channels: int | None = None, mask_value: float = 0.0, out: torch.Tensor | None = None,
                       scale: torch.Tensor | None = None, shift: torch.Tensor | None = None) -> torch.Tensor:
    """``gather_windows_augment`` for the features of a microphone array under its channel swaps (csrc/micswap.hip, DESIGN.md
    section 25): src [T, channels, 64] of ``kind`` 'logmel_gcc' (C + C(C-1)/2 channels) or 'logmel_nipd' (2C - 1);
    ``mic_perm``: int8 [16, C] host array (``seld_augment.mic_permutations``), row p the microphone permutation of pattern
    p or all -1 (no symmetry of the array: such a window is gathered untransformed).  Log-mel channels are copied, a
    GCC-PHAT pair that comes out of order has its lag axis reversed, an NIPD channel whose reference moved is the difference
    of two stored ones.  ``scale`` / ``shift`` and the masks as ``gather_windows_augment``."""
    import numpy as np
    src, index, starts, out = _window_call("gather_windows_mic", src, torch.float32, (None, N_MELS),
                                           "a float32 GPU tensor [T, C, 64]", starts, window, params, out)
    if kind not in MIC_KINDS:
        raise ValueError(f"gather_windows_mic: kind must be one of {sorted(MIC_KINDS)}, got {kind!r}")
    perm = np.ascontiguousarray(mic_perm, dtype=np.int8)
    if perm.ndim != 2 or perm.shape[0] != AUGMENT_PATTERNS:
        raise ValueError("gather_windows_mic: mic_perm must be int8 [16, microphones]")
    mics, channels = int(perm.shape[1]), int(src.shape[1])
    expected = mics + mics * (mics - 1) // 2 if kind == "logmel_gcc" else 2 * mics - 1
    if channels != expected:        # the library takes the channel count from (mics, kind): the source must have that many
        raise ValueError(f"gather_windows_mic: {kind!r} of {mics} microphones has {expected} feature channels, src has "
                         f"{channels}")
    freq_channels = channels if freq_channels is None else int(freq_channels)
    scale, shift = _affine_tables("gather_windows_mic", scale, shift, src)
    head = (_p(src), src.shape[0], mics, MIC_KINDS[kind], freq_channels, _p(starts), _p(params), starts.numel(), window,
            ctypes.c_void_p(perm.ctypes.data), float(mask_value))
    with _device_guard(index):
        if scale is not None:
            check(load_library().seld_window_gather_mic_standardised(*head, _p(scale), _p(shift), _p(out),
                                                               _stream_ptr(src.device)), "seld_window_gather_mic_standardised")
        else:
            check(load_library().seld_window_gather_mic(*head, _p(out), _stream_ptr(src.device)), "seld_window_gather_mic")
    return out


def foa_channels(order: str = "WYZX"):
    """(ch_x, ch_y, ch_z): the input channels that carry X, Y and Z under Config.FOA_CHANNEL_ORDER (W is channel 0)."""
    order = check_channel_order(order)
    return order.index("X"), order.index("Y"), order.index("Z")


def foa_rotation_terms(spec: torch.Tensor, order: str = "WYZX") -> torch.Tensor:
    """Rotation terms of the rotating gather (csrc/rotate.hip) from the complex STFT of 4-channel FOA clips, ``stft(pcm)``:
    complex64 [N, 4, F, 481] (or [4, F, 481]) -> float32 [N, F, 3, 64] time-major (or [F, 3, 64]):
    P_X = mel |X|^2, P_Y = mel |Y|^2, C = mel Re(X conj Y), linear (not dB)."""
    squeeze = spec.dim() == 3
    if squeeze:
        spec = spec.unsqueeze(0)
    if not spec.is_cuda or spec.dtype != torch.complex64 or spec.dim() != 4 or spec.shape[1] != 4 or spec.shape[3] != N_BINS:
        raise SeldNativeError("foa_rotation_terms: spec must be a complex64 GPU tensor [N, 4, F, 481]")
    ch_x, ch_y, _ = foa_channels(order)
    spec = spec.contiguous()
    n, _, frames, _ = spec.shape
    if n == 0 or frames == 0:
        raise ValueError("foa_rotation_terms: empty input")
    index = ensure_init(spec.device)
    out = torch.empty((n, frames, 3, N_MELS), dtype=torch.float32, device=spec.device)
    with _device_guard(index):
        check(load_library().seld_foa_rotation_terms(_p(torch.view_as_real(spec)), n, frames, ch_x, ch_y, _p(out),
                                                     frames * 3 * N_MELS, N_MELS, 1, 3 * N_MELS, _stream_ptr(spec.device)),
              "seld_foa_rotation_terms")
    return out[0] if squeeze else out


def gather_windows_rotate(src: torch.Tensor, rot: torch.Tensor, starts: torch.Tensor, window: int, params: torch.Tensor,
                          channel_table, order: str = "WYZX", J: int = GRID_J, freq_channels: int | None = None,
                          mask_value: float = 0.0, out: torch.Tensor | None = None, scale: torch.Tensor | None = None,
                          shift: torch.Tensor | None = None) -> torch.Tensor:
    """``gather_windows_augment`` with the azimuth step of ``params[:, 9]`` (csrc/rotate.hip): src [T, C, 64] with C = 4
    ('logmel') or 7 ('logmel_iv'), rot [T, 3, 64] the timeline's rotation terms (``foa_rotation_terms``).  A window whose
    total rotation is a whole number of quarter turns is the signed channel copy of ``gather_windows_augment``, bit for bit;
    any other window gets X' / Y' log-mel and IV_x' / IV_y' computed from the terms.  ``scale`` / ``shift``: as in
    ``gather_windows_augment`` (the standardising export; applied to the rotated values, before the masks)."""
    src, index, starts, out = _window_call("gather_windows_rotate", src, torch.float32, (None, N_MELS),
                                           "a float32 GPU tensor [T, C, 64]", starts, window, params, out)
    channels = int(src.shape[1])
    if not rot.is_cuda or rot.dtype != torch.float32 or tuple(rot.shape) != (src.shape[0], 3, N_MELS) or rot.device != src.device:
        raise SeldNativeError(f"gather_windows_rotate: rot must be a float32 tensor [{src.shape[0]}, 3, 64] on {src.device}")
    rot = rot.contiguous()
    ch_x, ch_y, ch_z = foa_channels(order)
    freq_channels = channels if freq_channels is None else int(freq_channels)
    table = _channel_table("gather_windows_rotate", channel_table, channels)
    scale, shift = _affine_tables("gather_windows_rotate", scale, shift, src)
    if scale is not None:
        with _device_guard(index):
            check(load_library().seld_window_gather_rotate_affine(
                _p(src), _p(rot), src.shape[0], channels, freq_channels, ch_x, ch_y, ch_z, int(J), _p(starts), _p(params),
                starts.numel(), window, ctypes.c_void_p(table.ctypes.data), float(mask_value), _p(scale), _p(shift), _p(out),
                _stream_ptr(src.device)), "seld_window_gather_rotate_affine")
        return out
    with _device_guard(index):
        check(load_library().seld_window_gather_rotate(
            _p(src), _p(rot), src.shape[0], channels, freq_channels, ch_x, ch_y, ch_z, int(J), _p(starts), _p(params),
            starts.numel(), window, ctypes.c_void_p(table.ctypes.data), float(mask_value), _p(out), _stream_ptr(src.device)),
            "seld_window_gather_rotate")
    return out


def gather_windows_permute_rotate(src: torch.Tensor, starts: torch.Tensor, window: int, params: torch.Tensor, I: int = GRID_I,
                                  J: int = GRID_J, out: torch.Tensor | None = None) -> torch.Tensor:
    """``gather_windows_permute`` with the azimuth index of every cell shifted by the window's total step
    (k J/4 + params[:, 9]) mod J after the mirror (csrc/rotate.hip)."""
    src, index, starts, out = _window_call("gather_windows_permute_rotate", src, torch.uint16, (I * J,),
                                           "a uint16 GPU tensor [T, I*J]", starts, window, params, out)
    with _device_guard(index):
        check(load_library().seld_window_permute_mask_rotate(_p(src), src.shape[0], I, J, _p(starts), _p(params),
                                                             starts.numel(), window, _p(out), _stream_ptr(src.device)),
              "seld_window_permute_mask_rotate")
    return out


def mix_partners(starts_b, patterns_b, gains, device) -> torch.Tensor:
    """The partner table of the mixing gathers (csrc/mix.hip) as an int64 [B, 2] device tensor, packed on the host and
    uploaded with one small asynchronous copy: row b = (start frame of the partner, fp32 bits of the linear power gain in
    bits 0..31 | the partner's spatial pattern in bits 32..35).  A gain of 0 means no partner.  The host table is checked --
    pattern in 0..15, gain finite and >= 0; the kernels clamp whatever a device table holds."""
    import numpy as np
    starts_b = np.asarray(starts_b, dtype=np.int64).reshape(-1)
    patterns_b = np.asarray(patterns_b, dtype=np.int64).reshape(-1)
    gains = np.asarray(gains, dtype=np.float32).reshape(-1)
    if not len(starts_b) == len(patterns_b) == len(gains):
        raise ValueError(f"mix partners: starts, patterns and gains must have one entry per window, got {len(starts_b)}, "
                         f"{len(patterns_b)} and {len(gains)}")
    if len(starts_b):
        if int(patterns_b.min()) < 0 or int(patterns_b.max()) >= AUGMENT_PATTERNS:
            raise ValueError("mix partners: spatial pattern outside 0..15")
        if not np.isfinite(gains).all() or float(gains.min()) < 0.0:
            raise ValueError("mix partners: a gain must be finite and >= 0 (0 = no partner)")
    table = np.empty((len(starts_b), 2), dtype=np.int64)
    table[:, 0] = starts_b
    table[:, 1] = gains.view(np.uint32).astype(np.int64) | (patterns_b << 32)
    return torch.from_numpy(table).to(device, non_blocking=True)


def _partner_table(name: str, partners: torch.Tensor, batch: int, device) -> torch.Tensor:
    if not (isinstance(partners, torch.Tensor) and partners.is_cuda and partners.device == device
            and partners.dtype == torch.int64 and partners.is_contiguous() and tuple(partners.shape) == (batch, 2)):
        raise ValueError(f"{name}: partners must be a contiguous int64 [B, 2] GPU tensor (mix_partners)")
    return partners


def gather_windows_mix(src: torch.Tensor, starts: torch.Tensor, window: int, params: torch.Tensor, partners: torch.Tensor,
                       channel_table=None, freq_channels: int | None = None, mask_value: float = 0.0, iv_channels: int = 0,
                       out: torch.Tensor | None = None, scale: torch.Tensor | None = None,
                       shift: torch.Tensor | None = None) -> torch.Tensor:
    """``gather_windows_augment`` where window b may be mixed with a partner window of the same timeline (csrc/mix.hip,
    DESIGN.md section 24): ``partners`` int64 [B, 2] on the device (``mix_partners``).  A frame without a partner row is
    the augmenting gather's, bit for bit; a mixed log-mel value is power_to_db(P_a + g P_b) on the stored dB values, each
    operand under its own spatial pattern; with ``iv_channels`` = 3 (C = 7, 'logmel_iv') channels 4..6 are intensity vectors,
    mixed with the band energies as weights.  ``scale`` / ``shift`` and the masks of ``params`` apply to the mixture."""
    src, index, starts, out = _window_call("gather_windows_mix", src, torch.float32, (None, N_MELS),
                                           "a float32 GPU tensor [T, C, 64]", starts, window, params, out)
    partners = _partner_table("gather_windows_mix", partners, starts.numel(), src.device)
    channels = int(src.shape[1])
    freq_channels = channels if freq_channels is None else int(freq_channels)
    table = None if channel_table is None else _channel_table("gather_windows_mix", channel_table, channels)
    table_p = ctypes.c_void_p(table.ctypes.data) if table is not None else None
    scale, shift = _affine_tables("gather_windows_mix", scale, shift, src)
    with _device_guard(index):
        if scale is not None:
            check(load_library().seld_window_gather_mix_standardised(
                _p(src), src.shape[0], channels, freq_channels, _p(starts), _p(params), _p(partners), starts.numel(), window,
                table_p, float(mask_value), int(iv_channels), _p(scale), _p(shift), _p(out), _stream_ptr(src.device)),
                "seld_window_gather_mix_standardised")
        else:
            check(load_library().seld_window_gather_mix(
                _p(src), src.shape[0], channels, freq_channels, _p(starts), _p(params), _p(partners), starts.numel(), window,
                table_p, float(mask_value), int(iv_channels), _p(out), _stream_ptr(src.device)), "seld_window_gather_mix")
    return out


def gather_windows_mix_mask(src: torch.Tensor, starts: torch.Tensor, window: int, params: torch.Tensor,
                            partners: torch.Tensor, I: int = GRID_I, J: int = GRID_J,
                            out: torch.Tensor | None = None) -> torch.Tensor:
    """``gather_windows_permute`` with the labels of each window's partner, moved by the partner's own pattern, ORed in
    (csrc/mix.hip): the class masks are bit masks, so the union is exact."""
    src, index, starts, out = _window_call("gather_windows_mix_mask", src, torch.uint16, (I * J,),
                                           "a uint16 GPU tensor [T, I*J]", starts, window, params, out)
    partners = _partner_table("gather_windows_mix_mask", partners, starts.numel(), src.device)
    with _device_guard(index):
        check(load_library().seld_window_mix_mask(_p(src), src.shape[0], I, J, _p(starts), _p(params), _p(partners),
                                                  starts.numel(), window, _p(out), _stream_ptr(src.device)),
              "seld_window_mix_mask")
    return out


def spectral_params(rows, curves, B: int, window: int, device):
    """The spectral rows and gain curves of the in-place stage (csrc/spectral.hip) on the device:
    (int32 [B, 12], float32 [B, 64] or None).  Host tables (numpy arrays / CPU tensors) are checked here -- |shift| <= 63,
    both cutouts inside the window and the 64 bins, curves finite -- and uploaded with one small asynchronous copy each;
    device tensors are trusted (no synchronise; the kernel clamps whatever it is given)."""
    t = torch.as_tensor(rows)
    if tuple(t.shape) != (B, SPECTRAL_PARAM_INTS):
        raise ValueError(f"spectral rows must be [{B}, {SPECTRAL_PARAM_INTS}], got {tuple(t.shape)}")
    if t.is_cuda:
        if t.dtype != torch.int32:
            raise TypeError("spectral rows on the device must be int32")
        t = t.contiguous()
    else:
        t = t.to(torch.int32).contiguous()
        if B:
            if int(t[:, 0].abs().max()) > N_MELS - 1:
                raise ValueError(f"spectral rows: frequency shift outside +-{N_MELS - 1} bins")
            for first in (2, 6):
                for axis, what, at in ((window, "frames", first), (N_MELS, "bins", first + 2)):
                    start, length = t[:, at], t[:, at + 1]
                    if int(start.min()) < 0 or int(length.min()) < 0 or int((start + length).max()) > axis:
                        raise ValueError(f"spectral rows: cutout outside the {axis} {what}")
        t = t.to(device, non_blocking=True)
    if curves is None:
        return t, None
    g = torch.as_tensor(curves)
    if tuple(g.shape) != (B, N_MELS):
        raise ValueError(f"gain curves must be [{B}, {N_MELS}], got {tuple(g.shape)}")
    if g.is_cuda:
        if g.dtype != torch.float32:
            raise TypeError("gain curves on the device must be float32")
        return t, g.contiguous()
    g = g.to(torch.float32).contiguous()
    if not bool(torch.isfinite(g).all()):
        raise ValueError("gain curves must be finite")
    return t, g.to(device, non_blocking=True)


def window_spectral(batch: torch.Tensor, starts: torch.Tensor, total_rows: int, params: torch.Tensor | None,
                    spectral: torch.Tensor, curves: torch.Tensor | None, logmel_channels: int, freq_channels: int,
                    mask_value: float = 0.0, scale: torch.Tensor | None = None, shift: torch.Tensor | None = None) -> torch.Tensor:
    """The in-place spectral stage on a gathered batch [B, window, C, 64] (float32, as a feature gather wrote it WITHOUT
    masks and WITHOUT ``scale`` / ``shift``; csrc/spectral.hip): per window the frequency shift of its
    spectral row (edge replication, channels < ``freq_channels``), its gain curve added to the log-mel channels (channels <
    ``logmel_channels``; the -100 dB floor kept), ``scale`` / ``shift`` (the map of the standardising gathers), the masks of
    ``params`` (None: no masks) and the two cutouts.  ``starts`` / ``total_rows``: what the gather was called with -- rows
    outside the timeline stay zero.  ``spectral`` / ``curves``: ``spectral_params``.  Returns ``batch``."""
    name = "window_spectral"
    if not (isinstance(batch, torch.Tensor) and batch.is_cuda and batch.dtype == torch.float32 and batch.dim() == 4
            and batch.shape[3] == N_MELS and batch.is_contiguous()):
        raise SeldNativeError(f"{name}: batch must be a contiguous float32 GPU tensor [B, window, C, 64]")
    B, window, channels = int(batch.shape[0]), int(batch.shape[1]), int(batch.shape[2])
    if window == 0 or channels == 0:
        raise ValueError(f"{name}: empty batch")
    index = ensure_init(batch.device)
    starts = starts.to(device=batch.device, dtype=torch.int64).contiguous()
    if starts.numel() != B:
        raise ValueError(f"{name}: starts must hold one frame per window, {B} here")
    for what, t, dtype, width in (("params", params, torch.int32, AUGMENT_PARAM_INTS),
                                  ("spectral", spectral, torch.int32, SPECTRAL_PARAM_INTS), ("curves", curves, torch.float32, N_MELS)):
        if t is None and what != "spectral":
            continue
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == batch.device and t.dtype == dtype
                and t.is_contiguous() and tuple(t.shape) == (B, width)):
            kind = str(dtype).replace("torch.", "")
            raise ValueError(f"{name}: {what} must be a contiguous {kind} [B, {width}] GPU tensor")
    if scale is None and shift is None:
        tables = None
    elif scale is None or shift is None:
        raise ValueError(f"{name}: scale and shift come together")
    else:
        for what, t in (("scale", scale), ("shift", shift)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == batch.device and t.dtype == torch.float32
                    and tuple(t.shape) == (channels, N_MELS)):
                raise SeldNativeError(f"{name}: {what} must be a float32 tensor {[channels, N_MELS]} on {batch.device}")
        tables = scale.contiguous(), shift.contiguous()
    head = (_p(batch), int(total_rows), channels, int(logmel_channels), int(freq_channels), _p(starts), _p(params), _p(spectral),
            _p(curves), B, window, float(mask_value))
    with _device_guard(index):
        if tables is not None:
            check(load_library().seld_window_spectral_standardised(*head, _p(tables[0]), _p(tables[1]),
                                                                   _stream_ptr(batch.device)), "seld_window_spectral_standardised")
        else:
            check(load_library().seld_window_spectral(*head, _stream_ptr(batch.device)), "seld_window_spectral")
    return batch


# --------------------------------------------------------------------------- fused loss

_workspaces = {}


def _workspace(device) -> torch.Tensor:
    key = (device.type, device.index)
    ws = _workspaces.get(key)
    if ws is None:
        ws = torch.empty(load_library().seld_softmax_mse_workspace_bytes(), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def _class_logits(name: str, logits: torch.Tensor) -> torch.Tensor:
    """The logits of a class-loss call, contiguous: a GPU tensor of float32 or bfloat16."""
    if not logits.is_cuda:
        raise SeldNativeError(f"{name}: logits must be a GPU tensor")
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{name}: logits must be float32 or bfloat16")
    return logits.contiguous()


def _class_labels(name: str, logits: torch.Tensor, labels: torch.Tensor, n_cells: int):
    """(labels contiguous, mask pointer, dense pointer) of a class-loss call: exactly one pointer is not None."""
    labels = labels.contiguous()
    if labels.dtype == torch.uint16:
        if labels.numel() != n_cells:
            raise ValueError(f"{name}: mask shape does not match logits")
        return labels, _p(labels), None
    if labels.dtype != torch.float32 or labels.numel() != logits.numel():
        raise ValueError(f"{name}: dense labels must be float32 with the logits' shape")
    return labels, None, _p(labels)


def softmax_mse(logits: torch.Tensor, labels: torch.Tensor, grad_scale: float | None = None):
    """loss.py:43-54 fused.  ``labels``: uint16 mask [...cells] or dense float32 [...cells, 14].
    Returns (loss scalar tensor, grad or None); grad has the dtype/shape of ``logits``."""
    logits = _class_logits("softmax_mse", logits)
    m = logits.shape[-1]
    n_cells = logits.numel() // m
    index = ensure_init(logits.device)
    labels, mask_p, dense_p = _class_labels("softmax_mse", logits, labels, n_cells)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    grad = torch.empty_like(logits) if grad_scale is not None else None
    with _device_guard(index):
        check(load_library().seld_softmax_mse(_p(logits), int(logits.dtype == torch.bfloat16), mask_p, dense_p,
                                              n_cells, m, float(grad_scale or 0.0), _p(loss), _p(grad),
                                              _p(_workspace(logits.device)), _stream_ptr(logits.device)),
              "seld_softmax_mse")
    return loss[0], grad


_ce_workspaces = {}


def softmax_ce(logits: torch.Tensor, labels: torch.Tensor, class_weights: torch.Tensor | None = None,
               focal_gamma: float = 0.0, grad_scale: float | None = None, return_weight_sum: bool = False):
    """loss.py:27-41 fused (csrc/loss_ce.hip): weighted cross-entropy against the labels' argmax, times q^focal_gamma with
    q the probability of the other classes (focal_gamma = 0: nn.CrossEntropyLoss(weight=class_weights)).  ``labels``: uint16
    mask [...cells] or dense float32 [...cells, 14]; ``class_weights``: 14 values on the logits' device, or None for ones.
    Returns (loss scalar tensor, grad or None[, W = sum of the cells' weights]); grad = grad_scale * d(loss)/d(logits) has the
    dtype/shape of ``logits``.  Nothing is read back: the call can be captured."""
    logits = _class_logits("softmax_ce", logits)
    m = logits.shape[-1]
    n_cells = logits.numel() // m
    index = ensure_init(logits.device)
    if logits.data_ptr() % 16:                # a view into a larger buffer: the kernels move 16-byte pieces
        logits = logits.clone()
    if labels.dtype != torch.uint16 and labels.is_contiguous() and labels.data_ptr() % 16:
        labels = labels.clone()
    labels, mask_p, dense_p = _class_labels("softmax_ce", logits, labels, n_cells)
    if class_weights is not None:
        if class_weights.device != logits.device or class_weights.numel() != m:
            raise ValueError(f"softmax_ce: class_weights must be {m} values on the logits' device")
        class_weights = class_weights.detach().to(torch.float32).contiguous()
    key = (logits.device.type, logits.device.index)
    ws = _ce_workspaces.get(key)
    if ws is None:
        ws = _ce_workspaces[key] = torch.empty(load_library().seld_softmax_ce_workspace_bytes(), dtype=torch.uint8,
                                               device=logits.device)
    out = torch.empty(2, dtype=torch.float32, device=logits.device)
    grad = torch.empty_like(logits) if grad_scale is not None else None
    with _device_guard(index):
        check(load_library().seld_softmax_ce(_p(logits), int(logits.dtype == torch.bfloat16), mask_p, dense_p, n_cells, m,
                                             _p(class_weights), float(focal_gamma), float(grad_scale or 0.0), _p(out),
                                             _p(grad), _p(ws), _stream_ptr(logits.device)), "seld_softmax_ce")
    return (out[0], grad, out[1]) if return_weight_sum else (out[0], grad)


def smr_loss(logits: torch.Tensor, labels: torch.Tensor, grid, w_class: float, w_aiur: float, w_cl: float,
             want_grad: bool):
    """smrl_seld_gaussian.py:946-1072 fused (csrc/loss3.hip).  logits [..., G, 14] with G = grid[0] * grid[1]; labels:
    uint16 mask [..., G] or dense float32 [..., G, 14].  Returns (terms [4] fp32 = total, mse, aiur, cl; grad like logits
    or None)."""
    logits = _class_logits("smr_loss", logits)
    rows, cols = int(grid[0]), int(grid[1])
    m = logits.shape[-1]
    cells = rows * cols
    if logits.dim() < 2 or logits.shape[-2] != cells:
        raise ValueError(f"smr_loss: logits must be [..., {cells}, {m}] for a {rows} x {cols} grid")
    frames = logits.numel() // (cells * m)
    labels, mask_p, dense_p = _class_labels("smr_loss", logits, labels, frames * cells)
    index = ensure_init(logits.device)
    lib = load_library()
    out = torch.empty(4, dtype=torch.float32, device=logits.device)
    grad = torch.empty_like(logits) if want_grad else None
    ws = torch.empty(lib.seld_smr_loss_workspace_bytes(frames, cells), dtype=torch.uint8, device=logits.device)
    with _device_guard(index):
        check(lib.seld_smr_loss(_p(logits), int(logits.dtype == torch.bfloat16), mask_p, dense_p, frames, rows, cols, m,
                                float(w_class), float(w_aiur), float(w_cl), _p(out), _p(grad), _p(ws),
                                _stream_ptr(logits.device)), "seld_smr_loss")
    return out, grad


_unit_gradients = {}        # device index -> a persistent ones scalar handed to autograd as the loss's upstream gradient


def unit_gradient(device) -> torch.Tensor:
    """The ones scalar ``loss.backward()`` would create with a fill kernel, kept per device: a caller that seeds the
    backward pass with it (``torch.autograd.backward(loss, unit_gradient(device))``) saves that launch, and
    ``scale_by_device_scalar_`` recognises it by address and skips its own (the upstream gradient IS one)."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    t = _unit_gradients.get(index)
    if t is None:
        t = _unit_gradients[index] = torch.ones((), dtype=torch.float32, device=device)
    return t


def scale_by_device_scalar_(data: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """data *= scale (a one-element fp32 GPU tensor) in place, without reading the scalar on the host; a scale of
    exactly 1.0 costs one empty launch.  Falls back to torch when the layout does not fit the kernel."""
    if scale.is_cuda and scale.numel() == 1:
        unit = _unit_gradients.get(scale.device.index)
        if unit is not None and scale.data_ptr() == unit.data_ptr():
            return data
    if (not data.is_cuda or data.dtype not in (torch.float32, torch.bfloat16) or not data.is_contiguous()
            or data.numel() % 8 or data.data_ptr() % 16 or scale.numel() != 1):
        return data.mul_(scale.to(data.dtype))
    scale = scale.reshape(1).to(device=data.device, dtype=torch.float32)
    with _device_guard(ensure_init(data.device)):
        check(load_library().seld_scale_by_device_scalar(_p(data), int(data.dtype == torch.bfloat16), data.numel(),
                                                         _p(scale), _stream_ptr(data.device)),
              "seld_scale_by_device_scalar")
    return data


def layernorm_supported(d: int) -> bool:
    return bool(load_library().seld_layernorm_supported(int(d)))


def _layernorm_refuse(what, x, weight, bias, dy, stats):
    """Name the argument the LayerNorm kernels cannot take (they read raw pointers: a wrong layout is silent garbage)."""
    def bad(msg):
        raise SeldNativeError(f"{what}: {msg}")
    if x.dtype not in (torch.float32, torch.bfloat16):
        bad(f"x must be float32 or bfloat16, got {x.dtype}")
    if x.dim() < 1 or x.shape[-1] == 0:
        bad(f"x must be [..., D], got {tuple(x.shape)}")
    if not x.is_contiguous():
        bad("x must be contiguous")
    d = x.shape[-1]
    others = [("weight", weight, (d,), torch.float32), ("bias", bias, (d,), torch.float32)]
    if dy is not None:
        others.append(("dy", dy, tuple(x.shape), x.dtype))
    if stats is not None:
        others.append(("stats", stats, (x.numel() // d, 2), torch.float32))
    for name, t, shape, dtype in others:
        if t.device != x.device:
            bad(f"{name} is on {t.device}, x on {x.device}")
        if t.dtype != dtype:
            bad(f"{name} must be {dtype}, got {t.dtype}")
        if tuple(t.shape) != shape:
            bad(f"{name} must be {shape}, got {tuple(t.shape)}")
        if not t.is_contiguous():
            bad(f"{name} must be contiguous")
    bad("arguments refused")


def _layernorm_ok(x, t, dtype):
    return t.dtype == dtype and t.device == x.device and t.is_contiguous()


def layernorm_forward(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float, relu: bool):
    """x [..., D] contiguous fp32 / bf16; weight, bias [D] fp32 contiguous, all on one device
    -> (y like x, mean_rstd [rows, 2] fp32).  Anything else is refused before a launch (SeldNativeError)."""
    d = x.shape[-1] if x.dim() else 0
    if not (d and x.dtype in (torch.float32, torch.bfloat16) and x.is_contiguous()
            and weight.shape == (d,) and bias.shape == (d,)
            and _layernorm_ok(x, weight, torch.float32) and _layernorm_ok(x, bias, torch.float32)):
        _layernorm_refuse("layernorm_forward", x, weight, bias, None, None)
    rows = x.numel() // d
    y = torch.empty_like(x)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    with _device_guard(ensure_init(x.device)):
        check(load_library().seld_layernorm_forward(_p(x), int(x.dtype == torch.bfloat16), rows, d, _p(weight), _p(bias),
                                                    float(eps), int(relu), _p(y), _p(stats), _stream_ptr(x.device)),
              "seld_layernorm_forward")
    return y, stats


def layernorm_backward(x: torch.Tensor, dy: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                       stats: torch.Tensor, relu: bool):
    """dy like x (dtype, shape, contiguous); stats [rows, 2] fp32 as layernorm_forward returned it
    -> (dx like x, dweight [D] fp32, dbias [D] fp32).  Anything else is refused before a launch (SeldNativeError)."""
    d = x.shape[-1] if x.dim() else 0
    if not (d and x.dtype in (torch.float32, torch.bfloat16) and x.is_contiguous()
            and weight.shape == (d,) and bias.shape == (d,) and dy.shape == x.shape
            and stats.shape == (x.numel() // d, 2)
            and _layernorm_ok(x, weight, torch.float32) and _layernorm_ok(x, bias, torch.float32)
            and _layernorm_ok(x, dy, x.dtype) and _layernorm_ok(x, stats, torch.float32)):
        _layernorm_refuse("layernorm_backward", x, weight, bias, dy, stats)
    rows = x.numel() // d
    lib = load_library()
    dx = torch.empty_like(x)
    dweight = torch.empty((d,), dtype=torch.float32, device=x.device)
    dbias = torch.empty((d,), dtype=torch.float32, device=x.device)
    work = torch.empty((lib.seld_layernorm_workspace_floats(rows, d),), dtype=torch.float32, device=x.device)
    with _device_guard(ensure_init(x.device)):
        check(lib.seld_layernorm_backward(_p(x), _p(dy), int(x.dtype == torch.bfloat16), rows, d, _p(weight), _p(bias),
                                          _p(stats), int(relu), _p(dx), _p(dweight), _p(dbias), _p(work),
                                          _stream_ptr(x.device)), "seld_layernorm_backward")
    return dx, dweight, dbias


def stream_delay(device, nanoseconds: int) -> None:
    """Hold the CURRENT stream of ``device`` for ``nanoseconds`` (seld_stream_delay)."""
    with _device_guard(ensure_init(device)):
        check(load_library().seld_stream_delay(int(nanoseconds), _stream_ptr(device)), "seld_stream_delay")


def _dense_like(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same shape and strides, and the storage is walked exactly once (contiguous in some memory format)."""
    if a.shape != b.shape or a.device != b.device:
        return False
    if any(sa != sb for sa, sb, n in zip(a.stride(), b.stride(), a.shape) if n > 1):     # size-1 dims: any stride
        return False
    return a.is_contiguous() or (a.dim() == 4 and a.is_contiguous(memory_format=torch.channels_last))


def multi_cast(srcs, dsts, cache=None) -> bool:
    """dsts[i] <- srcs[i] for lists of GPU tensors, bf16 -> fp32 or fp32 -> bf16 (all pairs the same direction), in one
    launch per 96 tensors (csrc/cast.hip).  Returns False -- having done nothing -- when a pair does not share its
    memory layout, so that the caller can fall back to the framework's copies.  ``cache``: a dict owned by a caller
    that passes the SAME parameter lists every iteration (the optimiser): the layout checks and the descriptor arrays
    are reused while every address is unchanged (the step is enqueue-bound: this is ~80 us of host time per call)."""
    srcs, dsts = list(srcs), list(dsts)
    if not srcs:
        return True
    if cache is not None:
        key = tuple(t.data_ptr() for t in srcs) + tuple(t.data_ptr() for t in dsts)
        hit = cache.get("key") == key
        if hit:
            src, dst, lengths, n, to_float = cache["args"]
            device = srcs[0].device
            with _device_guard(ensure_init(device)):
                check(load_library().seld_multi_cast(src, dst, lengths, n, to_float, _stream_ptr(device)),
                      "seld_multi_cast")
            return True
    to_float = srcs[0].dtype == torch.bfloat16
    want = (torch.bfloat16, torch.float32) if to_float else (torch.float32, torch.bfloat16)
    for s, d in zip(srcs, dsts):
        if s.dtype != want[0] or d.dtype != want[1] or not s.is_cuda or not _dense_like(s, d):
            return False
    n = len(srcs)
    src = (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs])
    dst = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dsts])
    lengths = (ctypes.c_int64 * n)(*[s.numel() for s in srcs])
    device = srcs[0].device
    if cache is not None:
        cache["key"], cache["args"] = key, (src, dst, lengths, n, int(to_float))
    with _device_guard(ensure_init(device)):
        check(load_library().seld_multi_cast(src, dst, lengths, n, int(to_float), _stream_ptr(device)), "seld_multi_cast")
    return True


def multi_adam(grads, params, exp_avgs, exp_avg_sqs, lows, lr: torch.Tensor, step: torch.Tensor, beta1: float, beta2: float,
               eps: float, weight_decay: float, grad_scale: float = 1.0, cache=None) -> bool:
    """One Adam update (csrc/adam.hip; the arithmetic of torch's fused Adam, L2 weight decay) of fp32 ``params`` from
    ``grads`` (bf16 or fp32, same layout as their parameter), rewriting the bf16 working copies ``lows[i]`` (or None) from
    the new values; ``lr`` / ``step`` are fp32 device scalars (``step`` already incremented).  Returns False -- having done
    nothing -- when a tensor does not qualify (layout / dtype), so that the caller can take the framework's path.
    ``cache``: dict of a caller that passes the same lists every iteration (descriptor arrays reused while no address
    changed; the key covers every cached address: grad, param, exp_avg, exp_avg_sq, low -- ``load_state_dict`` replaces
    the moment tensors while the gradients of the exchange path stay where they are)."""
    n = len(params)
    if n == 0:
        return True
    key = None
    if cache is not None:
        key = tuple(t.data_ptr() for t in grads) + tuple(t.data_ptr() for t in params) + \
            tuple(t.data_ptr() for t in exp_avgs) + tuple(t.data_ptr() for t in exp_avg_sqs) + \
            tuple(0 if t is None else t.data_ptr() for t in lows)
        if cache.get("key") == key:
            args = cache["args"]
        else:
            args = None
    else:
        args = None
    device = params[0].device
    if args is None:
        for g, p, m, v, lo in zip(grads, params, exp_avgs, exp_avg_sqs, lows):
            if not (p.is_cuda and p.dtype == torch.float32 and m.dtype == torch.float32 and v.dtype == torch.float32
                    and g.dtype in (torch.float32, torch.bfloat16) and _dense_like(g, p) and _dense_like(m, p)
                    and _dense_like(v, p) and (lo is None or (lo.dtype == torch.bfloat16 and _dense_like(lo, p)))):
                return False
        args = ((ctypes.c_void_p * n)(*[g.data_ptr() for g in grads]),
                (ctypes.c_int32 * n)(*[int(g.dtype == torch.bfloat16) for g in grads]),
                (ctypes.c_void_p * n)(*[p.data_ptr() for p in params]),
                (ctypes.c_void_p * n)(*[m.data_ptr() for m in exp_avgs]),
                (ctypes.c_void_p * n)(*[v.data_ptr() for v in exp_avg_sqs]),
                (ctypes.c_void_p * n)(*[0 if lo is None else lo.data_ptr() for lo in lows]),
                (ctypes.c_int64 * n)(*[p.numel() for p in params]))
        if cache is not None:
            cache["key"], cache["args"] = key, args
    if not (lr.is_cuda and step.is_cuda and lr.dtype == torch.float32 and step.dtype == torch.float32):
        return False
    with _device_guard(ensure_init(device)):
        check(load_library().seld_multi_adam(*args, n, _p(lr), _p(step), float(beta1), float(beta2), float(eps),
                                             float(weight_decay), float(grad_scale), _stream_ptr(device)), "seld_multi_adam")
    return True


# --------------------------------------------------------------------------- guarded update (csrc/guard.hip, adam.hip)

GUARD_WORDS = 8          # seld_guard_record (include/seld_hip.h): norm, coef, apply, skipped | steps_skipped, steps_clipped, 2 spare


def new_guard_record(device) -> torch.Tensor:
    """A zeroed seld_guard_record as a float32 tensor of 8 words (words 4 and 5 are int32 counters: ``read_guard``)."""
    return torch.zeros(GUARD_WORDS, dtype=torch.float32, device=device)


def read_guard(guard: torch.Tensor) -> dict:
    """The record on the host (ONE device-to-host copy, synchronises)."""
    host = guard.detach().cpu()
    counters = host.view(torch.int32)
    return {"grad_norm": float(host[0]), "clip_coef": float(host[1]), "apply": float(host[2]) != 0.0,
            "steps_skipped": int(counters[4]), "steps_clipped": int(counters[5])}


def grad_norm_scratch_floats(lengths) -> int:
    """Floats of partial scratch ``multi_grad_norm`` needs for tensors of these element counts."""
    lengths = [int(x) for x in lengths]
    out = ctypes.c_int64(0)
    check(load_library().seld_multi_grad_norm_scratch((ctypes.c_int64 * len(lengths))(*lengths), len(lengths),
                                                      ctypes.byref(out)), "seld_multi_grad_norm_scratch")
    return int(out.value)


def _guard_ok(guard) -> bool:
    return (guard.is_cuda and guard.dtype == torch.float32 and guard.is_contiguous() and guard.numel() >= GUARD_WORDS
            and guard.data_ptr() % 16 == 0)


def multi_grad_norm(grads, guard: torch.Tensor, partial: torch.Tensor, grad_scale: float = 1.0, max_norm: float = 0.0,
                    skip_nonfinite: bool = False, cache=None) -> bool:
    """Global L2 norm of ``grads`` (bf16 / fp32 GPU tensors, each dense in some memory format) times ``grad_scale``, the
    clip coefficient for ``max_norm`` (<= 0: exactly 1) and the apply / skip decision, written to ``guard`` (a
    ``new_guard_record``); ``partial``: fp32 scratch of ``grad_norm_scratch_floats`` elements.  Deterministic, no host
    synchronisation.  Returns False -- having done nothing -- when a tensor does not qualify.  ``cache``: dict of a caller
    that passes the same list every iteration (the key covers every address it caches)."""
    grads = list(grads)
    n = len(grads)
    if not (_guard_ok(guard) and partial.is_cuda and partial.dtype == torch.float32 and partial.is_contiguous()):
        return False
    key = args = None
    if cache is not None:
        key = tuple(g.data_ptr() for g in grads)
        if cache.get("key") == key:
            args = cache["args"]
    if args is None:
        for g in grads:
            if not (g.is_cuda and g.dtype in (torch.float32, torch.bfloat16) and g.numel() > 0 and _dense_like(g, g)):
                return False
        args = ((ctypes.c_void_p * n)(*[g.data_ptr() for g in grads]),
                (ctypes.c_int32 * n)(*[int(g.dtype == torch.bfloat16) for g in grads]),
                (ctypes.c_int64 * n)(*[g.numel() for g in grads]),
                sum((g.numel() + 4095) // 4096 for g in grads))
        if cache is not None:
            cache["key"], cache["args"] = key, args
    if args[3] > partial.numel():
        return False
    device = guard.device
    with _device_guard(ensure_init(device)):
        check(load_library().seld_multi_grad_norm(args[0], args[1], args[2], n, float(grad_scale), float(max_norm),
                                                  int(bool(skip_nonfinite)), _p(partial), partial.numel(), _p(guard),
                                                  _stream_ptr(device)), "seld_multi_grad_norm")
    return True


def multi_adam_guarded(grads, params, exp_avgs, exp_avg_sqs, lows, lr: torch.Tensor, step: torch.Tensor, beta1: float,
                       beta2: float, eps: float, weight_decay: float, grad_scale: float = 1.0, emas=None,
                       ema_decay: float = 0.0, guard=None, cache=None) -> bool:
    """``multi_adam`` behind a guard record (``multi_grad_norm``): nothing is written when ``guard`` says skip, the
    gradient is multiplied by its clip coefficient, and ``emas[i]`` (fp32, the parameter's layout; or None) follows the new
    master as ``ema += (1 - ema_decay) * (p - ema)`` in the same pass.  ``guard`` None: always apply, coefficient 1
    (EMA alone); ``emas`` None or ``ema_decay`` 0: no EMA.  Returns False -- having done nothing -- when a tensor does not
    qualify.  ``cache``: as for ``multi_adam``; the key covers every cached address (grad, param, exp_avg, exp_avg_sq,
    low, ema)."""
    n = len(params)
    if n == 0:
        return True
    if emas is None or float(ema_decay) == 0.0:
        emas = None
    if guard is not None and not _guard_ok(guard):
        return False
    key = args = None
    if cache is not None:
        key = tuple(t.data_ptr() for t in grads) + tuple(t.data_ptr() for t in params) + \
            tuple(t.data_ptr() for t in exp_avgs) + tuple(t.data_ptr() for t in exp_avg_sqs) + \
            tuple(0 if t is None else t.data_ptr() for t in lows) + \
            (() if emas is None else tuple(0 if t is None else t.data_ptr() for t in emas))
        if cache.get("key") == key:
            args = cache["args"]
    device = params[0].device
    if args is None:
        for i, (g, p, m, v, lo) in enumerate(zip(grads, params, exp_avgs, exp_avg_sqs, lows)):
            e = None if emas is None else emas[i]
            if not (p.is_cuda and p.dtype == torch.float32 and m.dtype == torch.float32 and v.dtype == torch.float32
                    and g.dtype in (torch.float32, torch.bfloat16) and _dense_like(g, p) and _dense_like(m, p)
                    and _dense_like(v, p) and (lo is None or (lo.dtype == torch.bfloat16 and _dense_like(lo, p)))
                    and (e is None or (e.dtype == torch.float32 and _dense_like(e, p)))):
                return False
        args = ((ctypes.c_void_p * n)(*[g.data_ptr() for g in grads]),
                (ctypes.c_int32 * n)(*[int(g.dtype == torch.bfloat16) for g in grads]),
                (ctypes.c_void_p * n)(*[p.data_ptr() for p in params]),
                (ctypes.c_void_p * n)(*[m.data_ptr() for m in exp_avgs]),
                (ctypes.c_void_p * n)(*[v.data_ptr() for v in exp_avg_sqs]),
                (ctypes.c_void_p * n)(*[0 if lo is None else lo.data_ptr() for lo in lows]),
                (ctypes.c_int64 * n)(*[p.numel() for p in params]),
                None if emas is None else (ctypes.c_void_p * n)(*[0 if e is None else e.data_ptr() for e in emas]))
        if cache is not None:
            cache["key"], cache["args"] = key, args
    if not (lr.is_cuda and step.is_cuda and lr.dtype == torch.float32 and step.dtype == torch.float32):
        return False
    with _device_guard(ensure_init(device)):
        check(load_library().seld_multi_adam_guarded(*args[:7], n, _p(lr), _p(step), float(beta1), float(beta2), float(eps),
                                                     float(weight_decay), float(grad_scale), args[7], float(ema_decay),
                                                     None if guard is None else _p(guard), _stream_ptr(device)),
              "seld_multi_adam_guarded")
    return True


# --------------------------------------------------------------------------- CNN block tail (BN + ReLU + pool)

def conv_tail_supported(channels: int) -> bool:
    return channels % 8 == 0 and 256 % (channels // 8) == 0


def _tail_view(x: torch.Tensor):
    """4-D activation in channels-last memory order -> (rows, C); raises when the memory order is anything else."""
    if x.dim() != 4 or not x.is_cuda or x.dtype not in (torch.float32, torch.bfloat16):
        raise SeldNativeError("conv_tail: x must be a 4-D GPU tensor of float32 or bfloat16")
    if not x.is_contiguous(memory_format=torch.channels_last):
        raise SeldNativeError("conv_tail: x must be in channels-last memory order")
    b, c, t, f = x.shape
    return b * t * f, c


def conv_tail_forward(x, weight, bias, running_mean, running_var, momentum, eps, training, pool, residual=None):
    """model_crnn.py:5-17 after the convolution: BatchNorm2d -> ReLU -> MaxPool2d((1, pool)) on a channels-last
    [B, C, T, F] activation; with ``residual`` (pool = 1): BatchNorm2d -> + residual -> ReLU (resnet50_model.py:30-52).
    Returns (y [B, C, T, F // pool] channels-last, mean_invstd [2, C], scale_shift [2, C])."""
    rows, c = _tail_view(x)
    if residual is not None:
        if pool != 1 or residual.shape != x.shape or residual.dtype != x.dtype:
            raise ValueError("conv_tail: the residual must match x and needs pool = 1")
        _tail_view(residual)
    b, _, t, f = x.shape
    width = 2 if pool == 2 else 1                   # pool = 4: no pooling, SiLU instead of ReLU (BatchNorm1d -> Swish)
    if f % width:
        raise ValueError("conv_tail: the frequency extent must be a multiple of the pool width")
    index = ensure_init(x.device)
    y = torch.empty((b, c, t, f // width), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    stats = torch.empty((2, 2, c), dtype=torch.float32, device=x.device)
    lib = load_library()
    ws = torch.empty(lib.seld_conv_tail_workspace_floats(c), dtype=torch.float32, device=x.device)
    with _device_guard(index):
        check(lib.seld_conv_tail_forward(_p(x), _p(residual), int(x.dtype == torch.bfloat16), rows, c, pool, _p(weight),
                                         _p(bias),
                                         _p(running_mean), _p(running_var), float(momentum), float(eps), int(training),
                                         _p(y), _p(stats[0]), _p(stats[1]), _p(ws), _stream_ptr(x.device)),
              "seld_conv_tail_forward")
    return y, stats[0], stats[1]


def conv_tail_forward_from_partials(x, partials, weight, bias, running_mean, running_var, momentum, eps, pool):
    """The training-mode ``conv_tail_forward`` without its statistics pass: ``partials`` [2, rows, C] fp32 holds plain
    sums of x and x^2 over disjoint parts of x (``conv3x3_forward(..., stats=True)``).  Same returns."""
    rows, c = _tail_view(x)
    lib = load_library()
    if not (partials.is_cuda and partials.dtype == torch.float32 and partials.dim() == 3 and partials.is_contiguous()
            and partials.shape[0] == 2 and partials.shape[2] == c
            and 1 <= partials.shape[1] <= lib.seld_conv_tail_partial_rows()):
        raise SeldNativeError("conv_tail: partials must be contiguous fp32 [2, rows <= 1024, C]")
    b, _, t, f = x.shape
    width = 2 if pool == 2 else 1
    if f % width:
        raise ValueError("conv_tail: the frequency extent must be a multiple of the pool width")
    index = ensure_init(x.device)
    y = torch.empty((b, c, t, f // width), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    stats = torch.empty((2, 2, c), dtype=torch.float32, device=x.device)
    with _device_guard(index):
        check(lib.seld_conv_tail_forward_from_partials(_p(x), int(x.dtype == torch.bfloat16), rows, c, pool, _p(partials),
                                                       partials.shape[1], _p(weight), _p(bias), _p(running_mean),
                                                       _p(running_var), float(momentum), float(eps), _p(y),
                                                       _p(stats[0]), _p(stats[1]), _stream_ptr(x.device)),
              "seld_conv_tail_forward_from_partials")
    return y, stats[0], stats[1]


def conv_tail_backward(x, dy, mean_invstd, scale_shift, pool, residual=None):
    """-> (dx like x, dweight [C] fp32, dbias [C] fp32[, dresidual like x when ``residual`` is given])."""
    rows, c = _tail_view(x)
    if dy.dtype != x.dtype or not dy.is_contiguous(memory_format=torch.channels_last):
        dy = dy.to(x.dtype).contiguous(memory_format=torch.channels_last)
    index = ensure_init(x.device)
    dx = torch.empty_like(x, memory_format=torch.channels_last)
    dres = torch.empty_like(x, memory_format=torch.channels_last) if residual is not None else None
    dwb = torch.empty((2, c), dtype=torch.float32, device=x.device)
    lib = load_library()
    ws = torch.empty(lib.seld_conv_tail_workspace_floats(c), dtype=torch.float32, device=x.device)
    with _device_guard(index):
        check(lib.seld_conv_tail_backward(_p(x), _p(residual), _p(dy), int(x.dtype == torch.bfloat16), rows, c, pool,
                                          _p(mean_invstd), _p(scale_shift), _p(dx), _p(dres), _p(dwb[0]), _p(dwb[1]),
                                          _p(ws), _stream_ptr(x.device)), "seld_conv_tail_backward")
    if residual is not None:
        return dx, dwb[0], dwb[1], dres
    return dx, dwb[0], dwb[1]


# --------------------------------------------------------------------------- depthwise Conv1d (Conformer conv module)

def dwconv1d_supported(d: int, k: int) -> bool:
    return d % 64 == 0 and 1 <= k <= 31 and k % 2 == 1


def dwconv1d(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, flip: bool = False) -> torch.Tensor:
    """Depthwise Conv1d over time on channels-last activations: x [B, T, D], weight [D, K] (fp32), bias [D] or None."""
    if not x.is_cuda or x.dim() != 3 or x.dtype not in (torch.float32, torch.bfloat16):
        raise SeldNativeError("dwconv1d: x must be a GPU tensor [B, T, D] of float32 or bfloat16")
    x = x.contiguous()
    b, t, d = x.shape
    w = weight.to(torch.float32).contiguous()
    bias = None if bias is None else bias.to(torch.float32).contiguous()
    y = torch.empty_like(x)
    with _device_guard(ensure_init(x.device)):
        check(load_library().seld_dwconv1d(_p(x), int(x.dtype == torch.bfloat16), _p(w), _p(bias), b, t, d, w.shape[1],
                                           int(flip), _p(y), _stream_ptr(x.device)), "seld_dwconv1d")
    return y


def dwconv1d_wgrad(x: torch.Tensor, dy: torch.Tensor, k: int):
    """-> (dweight [D, K] fp32, dbias [D] fp32) of the depthwise convolution."""
    x, dy = x.contiguous(), dy.to(x.dtype).contiguous()
    b, t, d = x.shape
    rows = int(load_library().seld_dwconv1d_wgrad_rows(b, t))          # one per batch row and 50-step time chunk
    partial = torch.empty((rows, d, 32), dtype=torch.float32, device=x.device)
    with _device_guard(ensure_init(x.device)):
        check(load_library().seld_dwconv1d_wgrad(_p(x), _p(dy), int(x.dtype == torch.bfloat16), b, t, d, k, _p(partial),
                                                 _stream_ptr(x.device)), "seld_dwconv1d_wgrad")
    total = partial.sum(dim=0)
    return total[:, :k], total[:, 31]


# --------------------------------------------------------------------------- GRU recurrence

GRU_H = 256
GRU_TILE = 2          # sequences per workgroup; set from seld_gru_tile_rows() by load_library()


def _tile_geometry():
    """(sequences per tile, lanes sharing a sequence, units per lane) of the loaded library: (8, 2, 4), (4, 4, 2) or
    (2, 8, 1).
    Without a built library (CPU-only checks of the torch layout definitions) the default build's geometry."""
    if LIB_PATH.exists():
        load_library()
    parts = 16 // GRU_TILE
    return GRU_TILE, parts, 8 // parts


def to_tile(x: torch.Tensor, ns: int) -> torch.Tensor:
    """[B, T, 2, ns, 256] -> the kernels' tile layout [tiles, T, 2, 8(w), ns, 4(q), parts, seqs, units] (batch
    zero-padded to whole tiles); the torch definition of what seld_gru_to_tile does.  Hidden unit
    u = 32*w + 16*s + 4*q + i with the flat index 4*s + i = part*units + j; row b = seqs*tile + seq; the lane
    dimensions (q, part, seq) are the wavefront lane q*16 + part*seqs + seq."""
    seqs, parts, units = _tile_geometry()
    b, t = x.shape[0], x.shape[1]
    tiles = (b + seqs - 1) // seqs
    if tiles * seqs != b:
        x = torch.cat((x, x.new_zeros((tiles * seqs - b,) + tuple(x.shape[1:]))), dim=0)
    x = x.reshape(tiles, seqs, t, 2, ns, 8, 2, 4, 4)                 # tile, seq, T, dir, slot, w, s, q, i
    x = x.permute(0, 2, 3, 5, 4, 7, 6, 8, 1)                         # tile, T, dir, w, slot, q, s, i, seq
    x = x.reshape(tiles, t, 2, 8, ns, 4, parts, units, seqs)         # (s, i) -> (part, j)
    return x.permute(0, 1, 2, 3, 4, 5, 6, 8, 7).contiguous()         # tile, T, dir, w, slot, q, part, seq, j


def from_tile(x: torch.Tensor, batch: int) -> torch.Tensor:
    """Inverse of to_tile: [tiles, T, 2, 8, ns, 4, parts, seqs, units] -> [batch, T, 2, ns, 256]."""
    seqs, parts, units = _tile_geometry()
    tiles, t, ns = x.shape[0], x.shape[1], x.shape[4]
    y = x.permute(0, 7, 1, 2, 4, 3, 5, 6, 8).reshape(tiles, seqs, t, 2, ns, 8, 4, 2, 4)   # .., w, q, s, i
    return y.permute(0, 1, 2, 3, 4, 5, 7, 6, 8).reshape(tiles * seqs, t, 2, ns, GRU_H)[:batch]


def from_pair_tile(x: torch.Tensor, batch: int):
    """The pair-slot layout of the backward kernel's output, [tiles, T, 2, 8(w), 2(pair slot), 4(q), parts, seqs,
    2(member), units] with slots (da_r|da_z), (da_n|da_n*r) -> (dgi [batch, T, 2, 3, 256] = (da_r, da_z, da_n),
    dghn [batch, T, 2, 256] = da_n*r); the torch definition of what seld_gru_from_pair_tile does."""
    seqs, parts, units = _tile_geometry()
    tiles, t = x.shape[0], x.shape[1]
    y = x.permute(0, 7, 1, 2, 4, 8, 3, 5, 6, 9).reshape(tiles, seqs, t, 2, 4, 8, 4, 2, 4)  # .., slot, w, q, s, i
    y = y.permute(0, 1, 2, 3, 4, 5, 7, 6, 8).reshape(tiles * seqs, t, 2, 4, GRU_H)[:batch]
    return y[:, :, :, :3].contiguous(), y[:, :, :, 3].contiguous()


def to_tile_device(x: torch.Tensor, ns: int) -> torch.Tensor:
    """``to_tile`` by the HIP permute kernel (x: contiguous GPU tensor [B, T, 2, ns, 256], bf16 or fp32)."""
    seqs, parts, units = _tile_geometry()
    b, t = x.shape[0], x.shape[1]
    tiles = (b + seqs - 1) // seqs
    x = x.contiguous()
    out = torch.empty((tiles, t, 2, 8, ns, 4, parts, seqs, units), dtype=x.dtype, device=x.device)
    with _device_guard(ensure_init(x.device)):
        check(load_library().seld_gru_to_tile(_p(x), x.element_size(), b, t, ns, _p(out), _stream_ptr(x.device)),
              "seld_gru_to_tile")
    return out


def from_pair_tile_device(x: torch.Tensor, batch: int):
    """``from_pair_tile`` by the HIP permute kernel."""
    t = x.shape[1]
    dgi = torch.empty((batch, t, 2, 3, GRU_H), dtype=x.dtype, device=x.device)
    dghn = torch.empty((batch, t, 2, GRU_H), dtype=x.dtype, device=x.device)
    with _device_guard(ensure_init(x.device)):
        check(load_library().seld_gru_from_pair_tile(_p(x), x.element_size(), batch, t, _p(dgi), _p(dghn),
                                                     _stream_ptr(x.device)), "seld_gru_from_pair_tile")
    return dgi, dghn


def gru_previous_state(y: torch.Tensor) -> torch.Tensor:
    """y [B, T, 2*256] (h_t of both directions) -> h_{t-1} in each direction's own time order, same shape; zero at the
    first step (t = 0 forward, t = T-1 reverse)."""
    b, t, _ = y.shape
    y = y.contiguous()
    out = torch.empty_like(y)
    with _device_guard(ensure_init(y.device)):
        check(load_library().seld_gru_previous_state(_p(y), y.element_size(), b, t, _p(out), _stream_ptr(y.device)),
              "seld_gru_previous_state")
    return out


def gru_forward(gi: torch.Tensor, w_hh: torch.Tensor, b_hn: torch.Tensor, need_saved: bool):
    """gi [B, T, 2, 3H] (fp32 / bf16; must already include b_ih and the r/z part of b_hh), w_hh [2, 3H, H],
    b_hn [2, H] (n-gate recurrent bias) -> (y [B, T, 2H], saved (tile layout, opaque) or None).  y is a view of
    the first B rows of a buffer padded to whole tiles of GRU_TILE sequences."""
    if not gi.is_cuda:
        raise SeldNativeError("gru_forward: tensors must live on the GPU")
    b, t, two, g3 = gi.shape
    h = g3 // 3
    if two != 2 or h != GRU_H or gi.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("gru_forward: gi must be [B, T, 2, 768] float32 or bfloat16")
    index = ensure_init(gi.device)
    gi = gi.contiguous()                    # read by the kernel as it is: the input GEMM's own output
    tiles = (b + GRU_TILE - 1) // GRU_TILE
    w = w_hh.to(torch.bfloat16).contiguous()
    bias = b_hn.to(torch.float32).contiguous()
    if tuple(bias.shape) != (2, h):
        raise ValueError("gru_forward: b_hn must be [2, H]")
    y = torch.empty((tiles * GRU_TILE, t, 2 * h), dtype=gi.dtype, device=gi.device)
    saved_dtype = torch.float16 if gi.dtype == torch.bfloat16 else torch.float32      # see include/seld_hip.h
    saved = torch.empty((tiles, t, 2, 8, 2, 64, 2, 8 * GRU_TILE // 16), dtype=saved_dtype, device=gi.device) \
        if need_saved else None
    with _device_guard(index):
        check(load_library().seld_gru_forward(_p(gi), int(gi.dtype == torch.bfloat16), _p(w), _p(bias), b, t,
                                              h, _p(y), _p(saved), _stream_ptr(gi.device)), "seld_gru_forward")
    return y[:b], saved


def gru_backward(dy: torch.Tensor, saved: torch.Tensor, y: torch.Tensor, w_hh: torch.Tensor, raw_bias: bool = False,
                 w_hh_t: torch.Tensor = None, direct: bool = True):
    """dy [B, T, 2H], the forward's (saved, y) -> (dgi [B, T, 2, 3, H] = (da_r, da_z, da_n), dghn [B, T, 2, H] =
    da_n*r, both of dy's dtype, dbias [2, 4, H] fp32 = the four slots summed over batch and time; with ``raw_bias``
    the per-tile sums [tiles, 2, 4, H] as the kernel left them, for ``gru_bias_grads``).  ``w_hh_t``: W_hh as bf16
    [2, H, 3H] if the caller has it already (``gru_prepare``), else it is formed here.  bf16 tensors go through the
    direct-layout kernel (one launch); fp32 ones, or ``direct=False``, through the layout converters and the tile kernel
    (three launches, same bits)."""
    b, t, h2 = dy.shape
    h = h2 // 2
    index = ensure_init(dy.device)
    if saved.dtype != (torch.float16 if dy.dtype == torch.bfloat16 else torch.float32):
        raise ValueError("gru_backward: saved activations do not belong to a forward pass of this dtype")
    if y.dtype != dy.dtype or tuple(y.shape) != (b, t, h2):
        raise ValueError("gru_backward: y must be the forward output matching dy")
    if w_hh_t is None:
        w_t = w_hh.to(torch.bfloat16).transpose(1, 2).contiguous()        # [2, H, 3H]
    else:
        if w_hh_t.dtype != torch.bfloat16 or tuple(w_hh_t.shape) != (2, h, 3 * h) or not w_hh_t.is_contiguous():
            raise ValueError("gru_backward: w_hh_t must be contiguous bf16 [2, H, 3H]")
        w_t = w_hh_t
    if direct and dy.dtype == torch.bfloat16 and GRU_TILE <= 4:           # (the 8-sequence build has no direct kernel)
        tiles = (b + GRU_TILE - 1) // GRU_TILE
        dy, y = dy.contiguous(), y.contiguous()
        dgi = torch.empty((b, t, 2, 3, h), dtype=dy.dtype, device=dy.device)
        dghn = torch.empty((b, t, 2, h), dtype=dy.dtype, device=dy.device)
        dbias = torch.empty((tiles, 2, 4, h), dtype=torch.float32, device=dy.device)
        with _device_guard(index):
            check(load_library().seld_gru_backward_direct(_p(dy), _p(saved), _p(y), 1, _p(w_t), b, t, h, _p(dgi), _p(dghn),
                                                          _p(dbias), _stream_ptr(dy.device)), "seld_gru_backward_direct")
        if raw_bias:
            return dgi, dghn, dbias
        return dgi, dghn, dbias.sum(dim=0) if tiles > 1 else dbias[0]
    dy_tile = to_tile_device(dy.reshape(b, t, 2, 1, h), 1)
    tiles = dy_tile.shape[0]
    if tiles * GRU_TILE != b:               # the kernel reads whole tiles of y (h_{t-1}); pad rows are never used
        y = torch.cat((y, y.new_zeros((tiles * GRU_TILE - b, t, h2))), dim=0)
    y = y.contiguous()
    dg_tile = torch.empty((tiles, t, 2, 8, 2, 4, 16 // GRU_TILE, GRU_TILE, 2, 8 * GRU_TILE // 16), dtype=dy.dtype,
                          device=dy.device)
    dbias = torch.empty((tiles, 2, 4, h), dtype=torch.float32, device=dy.device)
    with _device_guard(index):
        check(load_library().seld_gru_backward(_p(dy_tile), _p(saved), _p(y), int(dy.dtype == torch.bfloat16),
                                               _p(w_t), tiles, t, h, _p(dg_tile), _p(dbias), _stream_ptr(dy.device)),
              "seld_gru_backward")
    dgi, dghn = from_pair_tile_device(dg_tile, b)
    if raw_bias:
        return dgi, dghn, dbias
    return dgi, dghn, dbias.sum(dim=0) if tiles > 1 else dbias[0]


# --------------------------------------------------------------------------- glue kernels (csrc/glue.hip)

def _is_bf16(t: torch.Tensor) -> int:
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"float32 or bfloat16 expected, got {t.dtype}")
    return int(t.dtype == torch.bfloat16)


def gru_fold_bias(b_ih: torch.Tensor, b_hh: torch.Tensor, dtype: torch.dtype):
    """b_ih, b_hh: fp32 [2*3H] (forward rows, then reverse) -> (gi_bias [6H] in ``dtype`` = b_ih + the r / z rows of b_hh,
    b_hn [2, H] fp32): one launch instead of clone, fill, add, cast, slice-copy."""
    if not (b_ih.is_cuda and b_ih.dtype == torch.float32 and b_hh.dtype == torch.float32 and b_ih.is_contiguous()
            and b_hh.is_contiguous() and b_ih.numel() == b_hh.numel() and b_ih.numel() % 6 == 0):
        raise SeldNativeError("gru_fold_bias: b_ih, b_hh must be contiguous fp32 GPU tensors of 2 * 3H elements")
    h = b_ih.numel() // 6
    gi_bias = torch.empty(6 * h, dtype=dtype, device=b_ih.device)
    b_hn = torch.empty((2, h), dtype=torch.float32, device=b_ih.device)
    with _device_guard(ensure_init(b_ih.device)):
        check(load_library().seld_gru_fold_bias(_p(b_ih), _p(b_hh), h, _p(gi_bias), _is_bf16(gi_bias), _p(b_hn),
                                                _stream_ptr(b_ih.device)), "seld_gru_fold_bias")
    return gi_bias, b_hn


def gru_prepare(b_ih: torch.Tensor, b_hh: torch.Tensor, w_hh: torch.Tensor, dtype: torch.dtype):
    """``gru_fold_bias`` plus, in the same launch, W_hh [2, 3H, H] (fp32 or bf16, contiguous) as the backward
    recurrence reads it: bf16 [2, H, 3H] -> (gi_bias, b_hn, w_hh_t)."""
    if not (b_ih.is_cuda and b_ih.dtype == torch.float32 and b_hh.dtype == torch.float32 and b_ih.is_contiguous()
            and b_hh.is_contiguous() and b_ih.numel() == b_hh.numel() and b_ih.numel() % 6 == 0):
        raise SeldNativeError("gru_prepare: b_ih, b_hh must be contiguous fp32 GPU tensors of 2 * 3H elements")
    h = b_ih.numel() // 6
    if not (w_hh.is_cuda and w_hh.is_contiguous() and tuple(w_hh.shape) == (2, 3 * h, h) and h % 32 == 0):
        raise SeldNativeError("gru_prepare: w_hh must be a contiguous GPU tensor [2, 3H, H], H a multiple of 32")
    gi_bias = torch.empty(6 * h, dtype=dtype, device=b_ih.device)
    b_hn = torch.empty((2, h), dtype=torch.float32, device=b_ih.device)
    w_t = torch.empty((2, h, 3 * h), dtype=torch.bfloat16, device=b_ih.device)
    with _device_guard(ensure_init(b_ih.device)):
        check(load_library().seld_gru_prepare(_p(b_ih), _p(b_hh), _p(w_hh), _is_bf16(w_hh), h, _p(gi_bias),
                                              _is_bf16(gi_bias), _p(b_hn), _p(w_t), _stream_ptr(b_ih.device)),
              "seld_gru_prepare")
    return gi_bias, b_hn, w_t


def gru_bias_grads(partial: torch.Tensor, out=None):
    """The backward recurrence's per-tile sums [tiles, 2, 4, H] fp32 -> (db_ih [2*3H], db_hh [2*3H]) fp32; written
    into ``out = (db_ih, db_hh)`` (contiguous fp32, 6H elements each) when given."""
    tiles, two, four, h = partial.shape
    if two != 2 or four != 4 or partial.dtype != torch.float32 or not partial.is_contiguous():
        raise SeldNativeError("gru_bias_grads: partial must be contiguous fp32 [tiles, 2, 4, H]")
    if out is None:
        db = torch.empty((2, 6 * h), dtype=torch.float32, device=partial.device)
        out = (db[0], db[1])
    elif not all(o.dtype == torch.float32 and o.is_contiguous() and o.numel() == 6 * h and o.device == partial.device
                 for o in out):
        raise SeldNativeError("gru_bias_grads: out must be two contiguous fp32 tensors of 6H elements")
    with _device_guard(ensure_init(partial.device)):
        check(load_library().seld_gru_bias_grads(_p(partial), tiles, h, _p(out[0]), _p(out[1]),
                                                 _stream_ptr(partial.device)), "seld_gru_bias_grads")
    return out[0], out[1]


def sum_chunks(partial: torch.Tensor, out: torch.Tensor, columns_cf=None) -> torch.Tensor:
    """out[...] = partial.sum(dim=0) accumulated in fp32 (partial [chunks, ...] contiguous bf16 / fp32; out contiguous).
    ``columns_cf = (C, F)``: partial is [chunks, rows, F * C] with columns ordered f * C + c and out [rows, C * F] gets
    them ordered c * F + f -- the same bits as the plain sum followed by that column permutation, in one launch."""
    if not (partial.is_cuda and partial.is_contiguous() and out.is_contiguous()
            and tuple(partial.shape[1:]) == tuple(out.shape)):
        raise SeldNativeError("sum_chunks: partial [chunks, ...] and out [...] must be contiguous with matching shapes")
    with _device_guard(ensure_init(partial.device)):
        if columns_cf is None:
            check(load_library().seld_sum_chunks(_p(partial), _is_bf16(partial), partial.shape[0], out.numel(), _p(out),
                                                 _is_bf16(out), _stream_ptr(partial.device)), "seld_sum_chunks")
        else:
            c, f = columns_cf
            if out.dim() != 2 or out.shape[1] != c * f:
                raise SeldNativeError("sum_chunks: columns_cf = (C, F) needs out [rows, C * F]")
            check(load_library().seld_sum_chunks_columns(_p(partial), _is_bf16(partial), partial.shape[0], out.shape[0],
                                                         c, f, _p(out), _is_bf16(out), _stream_ptr(partial.device)),
                  "seld_sum_chunks_columns")
    return out


def column_sums_supported(g: torch.Tensor, out: torch.Tensor) -> bool:
    return (g.is_cuda and g.dim() == 2 and g.is_contiguous() and out.is_contiguous() and g.shape[1] % 8 == 0
            and g.dtype in (torch.float32, torch.bfloat16) and out.dtype in (torch.float32, torch.bfloat16)
            and out.numel() == g.shape[1] and g.data_ptr() % 16 == 0 and g.shape[0] > 0)


def column_sums(g: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[n] = sum_r g[r, n] accumulated in fp32 (the bias gradient of a Linear from its [rows, N] output gradient)."""
    if not column_sums_supported(g, out):
        raise SeldNativeError("column_sums: g [rows, N] contiguous bf16 / fp32 with N % 8 == 0, out [N] contiguous")
    lib = load_library()
    rows, n = g.shape
    blocks = int(lib.seld_column_sums_blocks(rows, n))
    partial = torch.empty((blocks, n), dtype=torch.float32, device=g.device)
    with _device_guard(ensure_init(g.device)):
        check(lib.seld_column_sums(_p(g), _is_bf16(g), rows, n, _p(partial), _p(out), _is_bf16(out), _stream_ptr(g.device)),
              "seld_column_sums")
    return out


def multi_sum_chunks(pairs) -> None:
    """``out[...] = partial.sum(dim=0)`` for every (partial [chunks, ...], out [...]) pair in ONE launch per 64 pairs
    (csrc/glue.hip multi_sum_chunks_kernel; fp32 accumulation in chunk order, like ``sum_chunks``)."""
    pairs = list(pairs)
    if not pairs:
        return
    for partial, out in pairs:
        if not (partial.is_cuda and partial.is_contiguous() and out.is_contiguous()
                and tuple(partial.shape[1:]) == tuple(out.shape) and partial.dtype in (torch.float32, torch.bfloat16)
                and out.dtype in (torch.float32, torch.bfloat16)):
            raise SeldNativeError("multi_sum_chunks: partial [chunks, ...] / out [...] contiguous bf16 or fp32")
    n = len(pairs)
    src = (ctypes.c_void_p * n)(*[p.data_ptr() for p, _ in pairs])
    dst = (ctypes.c_void_p * n)(*[o.data_ptr() for _, o in pairs])
    counts = (ctypes.c_int64 * n)(*[o.numel() for _, o in pairs])
    chunks = (ctypes.c_int32 * n)(*[p.shape[0] for p, _ in pairs])
    flags = (ctypes.c_int32 * n)(*[_is_bf16(p) | (_is_bf16(o) << 1) for p, o in pairs])
    device = pairs[0][1].device
    with _device_guard(ensure_init(device)):
        check(load_library().seld_multi_sum_chunks(src, dst, counts, chunks, flags, n, _stream_ptr(device)),
              "seld_multi_sum_chunks")


_column_scratch = {}      # device index -> fp32 scratch for the row-block partials, grown on demand
_retired_scratch = []


def multi_column_sums(pairs) -> None:
    """``out[n] = sum_r g[r, n]`` for every (g [rows, N], out [N]) pair in TWO launches per 40 pairs (csrc/glue.hip
    multi_column_partials_kernel / multi_column_finish_kernel: row blocks in parallel, added in a fixed order)."""
    pairs = list(pairs)
    if not pairs:
        return
    for g, out in pairs:
        if not column_sums_supported(g, out):
            raise SeldNativeError("multi_column_sums: g [rows, N] contiguous bf16 / fp32 with N % 8 == 0, out [N] contiguous")
    lib = load_library()
    n = len(pairs)
    src = (ctypes.c_void_p * n)(*[g.data_ptr() for g, _ in pairs])
    dst = (ctypes.c_void_p * n)(*[o.data_ptr() for _, o in pairs])
    rows = (ctypes.c_int64 * n)(*[g.shape[0] for g, _ in pairs])
    cols = (ctypes.c_int64 * n)(*[g.shape[1] for g, _ in pairs])
    flags = (ctypes.c_int32 * n)(*[_is_bf16(g) | (_is_bf16(o) << 1) for g, o in pairs])
    need_f = ctypes.c_int64(0)
    check(lib.seld_multi_column_sums_scratch(rows, cols, n, ctypes.byref(need_f)), "seld_multi_column_sums_scratch")
    device = pairs[0][0].device
    index = ensure_init(device)
    scratch = _column_scratch.get(index)
    if scratch is None or scratch.numel() < need_f.value:
        if torch.cuda.is_current_stream_capturing():
            raise SeldNativeError("multi_column_sums: the scratch must be sized by an eager call before a graph capture")
        if scratch is not None:
            _retired_scratch.append(scratch)          # a captured graph may still hold its address: never handed back
        scratch = torch.empty(max(need_f.value, 1 << 20), dtype=torch.float32, device=device)
        _column_scratch[index] = scratch
    with _device_guard(index):
        check(lib.seld_multi_column_sums(src, dst, rows, cols, flags, n, _p(scratch), scratch.numel(), _stream_ptr(device)),
              "seld_multi_column_sums")


def gru_dwhh_finish(p_gi: torch.Tensor, p_n: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """p_gi [chunks, 6H, 2H], p_n [chunks, 2H, 2H] (chunked products against both directions' h_prev) -> out [2, 3H, H]."""
    chunks = p_gi.shape[0]
    h = out.shape[2]
    if not (p_gi.is_contiguous() and p_n.is_contiguous() and out.is_contiguous() and p_gi.dtype == p_n.dtype
            and tuple(p_gi.shape) == (chunks, 6 * h, 2 * h) and tuple(p_n.shape) == (chunks, 2 * h, 2 * h)
            and tuple(out.shape) == (2, 3 * h, h)):
        raise SeldNativeError("gru_dwhh_finish: shapes must be [chunks, 6H, 2H], [chunks, 2H, 2H] -> [2, 3H, H]")
    with _device_guard(ensure_init(out.device)):
        check(load_library().seld_gru_dwhh_finish(_p(p_gi), _p(p_n), _is_bf16(p_gi), chunks, h, _p(out), _is_bf16(out),
                                                  _stream_ptr(out.device)), "seld_gru_dwhh_finish")
    return out


def conv_weight_flip_transpose(w: torch.Tensor) -> torch.Tensor:
    """w [O, I, 3, 3] in channels-last memory -> [I, O, 3, 3] in channels-last memory with wt[i,o,r,s] = w[o,i,2-r,2-s]
    (= ``w.transpose(0, 1).flip(2, 3).contiguous(memory_format=torch.channels_last)`` in one launch)."""
    o, i, kh, kw = w.shape
    if not (w.is_cuda and kh == 3 and kw == 3 and w.dtype in (torch.float32, torch.bfloat16)
            and w.is_contiguous(memory_format=torch.channels_last)):
        raise SeldNativeError("conv_weight_flip_transpose: 3x3 weights in channels-last memory expected")
    wt = torch.empty((i, o, 3, 3), dtype=w.dtype, device=w.device, memory_format=torch.channels_last)
    with _device_guard(ensure_init(w.device)):
        check(load_library().seld_conv_weight_flip_transpose(_p(w), w.element_size(), o, i, _p(wt),
                                                             _stream_ptr(w.device)), "seld_conv_weight_flip_transpose")
    return wt


def conv3x3_wgrad_applicable(x: torch.Tensor, dy: torch.Tensor, w: torch.Tensor) -> bool:
    """True when ``conv3x3_wgrad`` covers this 3x3 / stride 1 / pad 1 convolution: bf16 x [B, Cin, T, F] and
    dy [B, Cout, T, F] in channels-last memory, F in {8, 16, 32}, channel counts multiples of 64, and weights
    [Cout, Cin, 3, 3] in channels-last memory (the gradient is written in that layout)."""
    if not (x.is_cuda and x.dim() == 4 and dy.dim() == 4 and w.dim() == 4 and x.dtype == torch.bfloat16
            and dy.dtype == torch.bfloat16 and tuple(w.shape[2:]) == (3, 3)):
        return False
    b, cin, t, f = x.shape
    if tuple(dy.shape) != (b, w.shape[0], t, f) or w.shape[1] != cin:
        return False
    if not (x.is_contiguous(memory_format=torch.channels_last) and dy.is_contiguous(memory_format=torch.channels_last)
            and w.is_contiguous(memory_format=torch.channels_last)):
        return False
    return bool(load_library().seld_conv3x3_wgrad_supported(f, cin, w.shape[0]))


def conv3x3_wgrad(x: torch.Tensor, dy: torch.Tensor, dw: torch.Tensor) -> torch.Tensor:
    """dw [Cout, Cin, 3, 3] (channels-last memory, bf16 or fp32) = the weight gradient of a 3x3 / stride 1 / pad 1
    bias-free convolution with input x and output gradient dy (both bf16, channels-last; ``conv3x3_wgrad_applicable``).
    fp32 accumulation, one rounding; deterministic.  The fp32 workspace comes from the caching allocator on the
    current stream."""
    if not conv3x3_wgrad_applicable(x, dy, dw) or dw.dtype not in (torch.float32, torch.bfloat16):
        raise SeldNativeError("conv3x3_wgrad: unsupported shapes, dtypes or layouts")
    b, cin, t, f = x.shape
    cout = dy.shape[1]
    with _device_guard(ensure_init(x.device)):
        lib = load_library()
        ws = torch.empty(int(lib.seld_conv3x3_wgrad_workspace_floats(b, t, f, cin, cout)), dtype=torch.float32,
                         device=x.device)
        check(lib.seld_conv3x3_wgrad(_p(x), _p(dy), b, t, f, cin, cout, _p(dw), _is_bf16(dw), _p(ws),
                                     _stream_ptr(x.device)), "seld_conv3x3_wgrad")
    return dw


def conv3x3_dgrad_applicable(dy: torch.Tensor, w: torch.Tensor) -> bool:
    """True when ``conv3x3_dgrad`` covers this 3x3 / stride 1 / pad 1 convolution: bf16 dy [B, Cout, T, F] and bf16
    weights [Cout, Cin, 3, 3], both in channels-last memory, F in {8, 16, 32}, channel counts multiples of 64."""
    if not (dy.is_cuda and dy.dim() == 4 and w.dim() == 4 and dy.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
            and tuple(w.shape[2:]) == (3, 3) and dy.shape[1] == w.shape[0]):
        return False
    if not (dy.is_contiguous(memory_format=torch.channels_last) and w.is_contiguous(memory_format=torch.channels_last)):
        return False
    return bool(load_library().seld_conv3x3_dgrad_supported(dy.shape[3], w.shape[1], w.shape[0]))


def conv3x3_dgrad(dy: torch.Tensor, w: torch.Tensor, out: "torch.Tensor | None" = None) -> torch.Tensor:
    """dx [B, Cin, T, F] (bf16, channels-last memory; ``out`` when given) = the data gradient of a 3x3 / stride 1 /
    pad 1 bias-free convolution with weights w and output gradient dy (``conv3x3_dgrad_applicable``), read from w as it
    lies: no flipped, transposed copy.  fp32 accumulation, one rounding; deterministic."""
    if not conv3x3_dgrad_applicable(dy, w):
        raise SeldNativeError("conv3x3_dgrad: unsupported shapes, dtypes or layouts")
    b, cout, t, f = dy.shape
    cin = w.shape[1]
    if out is None:
        out = torch.empty((b, cin, t, f), dtype=torch.bfloat16, device=dy.device, memory_format=torch.channels_last)
    elif not (out.dtype == torch.bfloat16 and out.device == dy.device and tuple(out.shape) == (b, cin, t, f)
              and out.is_contiguous(memory_format=torch.channels_last)):
        raise SeldNativeError("conv3x3_dgrad: out must be bf16 [B, Cin, T, F] in channels-last memory")
    with _device_guard(ensure_init(dy.device)):
        check(load_library().seld_conv3x3_dgrad(_p(dy), _p(w), b, t, f, cin, cout, _p(out), _stream_ptr(dy.device)),
              "seld_conv3x3_dgrad")
    return out


def conv3x3_forward_applicable(x: torch.Tensor, w: torch.Tensor) -> bool:
    """True when ``conv3x3_forward`` covers this 3x3 / stride 1 / pad 1 convolution: bf16 x [B, Cin, T, F] and bf16
    weights [Cout, Cin, 3, 3], both in channels-last memory, F in {8, 16, 32}, channel counts multiples of 64."""
    if not (x.is_cuda and x.dim() == 4 and w.dim() == 4 and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
            and tuple(w.shape[2:]) == (3, 3) and x.shape[1] == w.shape[1]):
        return False
    if not (x.is_contiguous(memory_format=torch.channels_last) and w.is_contiguous(memory_format=torch.channels_last)):
        return False
    return bool(load_library().seld_conv3x3_forward_supported(x.shape[3], w.shape[1], w.shape[0]))


def conv3x3_forward_supported(f: int, cin: int, cout: int) -> bool:
    return bool(load_library().seld_conv3x3_forward_supported(f, cin, cout))


def conv_tail_partial_rows() -> int:
    """Partial rows per statistic the tail's finalise step takes."""
    return int(load_library().seld_conv_tail_partial_rows())


def conv3x3_forward_chunks(b: int, t: int, f: int) -> int:
    """Partial rows ``conv3x3_forward(..., stats=True)`` writes: chunks of 256 positions, whole time rows of one clip."""
    return int(load_library().seld_conv3x3_forward_chunks(b, t, f))


def conv3x3_forward(x: torch.Tensor, w: torch.Tensor, stats: bool = False, out: "torch.Tensor | None" = None,
                    partials: "torch.Tensor | None" = None):
    """y [B, Cout, T, F] (bf16, channels-last memory; ``out`` when given) = the 3x3 / stride 1 / pad 1 bias-free
    convolution of x with w (``conv3x3_forward_applicable``), the weights read as they lie.  fp32 accumulation, one
    rounding; deterministic.  ``stats``: also returns partials [2, chunks, Cout] fp32 (``partials`` when given), the
    per-chunk sums of the stored y and y^2 per channel."""
    if not conv3x3_forward_applicable(x, w):
        raise SeldNativeError("conv3x3_forward: unsupported shapes, dtypes or layouts")
    b, cin, t, f = x.shape
    cout = w.shape[0]
    if out is None:
        out = torch.empty((b, cout, t, f), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    elif not (out.dtype == torch.bfloat16 and out.device == x.device and tuple(out.shape) == (b, cout, t, f)
              and out.is_contiguous(memory_format=torch.channels_last)):
        raise SeldNativeError("conv3x3_forward: out must be bf16 [B, Cout, T, F] in channels-last memory")
    with _device_guard(ensure_init(x.device)):
        lib = load_library()
        if stats:
            shape = (2, int(lib.seld_conv3x3_forward_chunks(b, t, f)), cout)
            if partials is None:
                partials = torch.empty(shape, dtype=torch.float32, device=x.device)
            elif not (partials.dtype == torch.float32 and partials.device == x.device and tuple(partials.shape) == shape
                      and partials.is_contiguous()):
                raise SeldNativeError("conv3x3_forward: partials must be contiguous fp32 [2, chunks, Cout]")
        else:
            partials = None
        check(lib.seld_conv3x3_forward(_p(x), _p(w), b, t, f, cin, cout, _p(out), _p(partials), _stream_ptr(x.device)),
              "seld_conv3x3_forward")
    return (out, partials) if stats else out


# --------------------------------------------------------------------------- first encoder block (conv recomputed)

def convfirst_applicable(x: torch.Tensor, w: torch.Tensor) -> bool:
    """True when ``convfirst_forward`` covers this block input: bf16 x [B, 4, T, F] in channels-last memory,
    w [64, 4, 3, 3] (bf16 or fp32, any strides), F a power of two in 16 .. 256."""
    if not (x.is_cuda and x.dim() == 4 and w.dim() == 4 and x.dtype == torch.bfloat16
            and w.dtype in (torch.float32, torch.bfloat16) and tuple(w.shape[2:]) == (3, 3) and w.shape[1] == x.shape[1]
            and x.is_contiguous(memory_format=torch.channels_last)):
        return False
    return bool(load_library().seld_convfirst_supported(x.shape[3], x.shape[1], w.shape[0]))


def convfirst_forward(x, w, bn_weight, bn_bias, running_mean, running_var, momentum, eps, phases=3):
    """Conv3x3(4 -> 64) -> BatchNorm2d (training) -> ReLU -> MaxPool2d((1, 2)) with the convolution recomputed in both
    passes (csrc/convfirst.hip).  Returns (y [B, 64, T, F // 2] bf16 channels-last, mean_invstd [2, 64], scale_shift
    [2, 64]); the running statistics are updated in place."""
    if not convfirst_applicable(x, w):
        raise SeldNativeError("convfirst: unsupported shapes, dtypes or layouts")
    b, _, t, f = x.shape
    index = ensure_init(x.device)
    y = torch.empty((b, w.shape[0], t, f // 2), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    stats = torch.empty((2, 2, w.shape[0]), dtype=torch.float32, device=x.device)
    lib = load_library()
    ws = torch.empty(int(lib.seld_convfirst_workspace_floats(0)), dtype=torch.float32, device=x.device)
    with _device_guard(index):
        check(lib.seld_convfirst_forward(_p(x), _p(w), _is_bf16(w), *w.stride(), b, t, f, _p(bn_weight), _p(bn_bias),
                                         _p(running_mean), _p(running_var), float(momentum), float(eps), _p(y),
                                         _p(stats[0]), _p(stats[1]), _p(ws), int(phases), _stream_ptr(x.device)),
              "seld_convfirst_forward")
    return y, stats[0], stats[1]


def convfirst_backward(x, w, dy, mean_invstd, scale_shift, dw, phases=3):
    """-> (dw, dgamma [64] fp32, dbeta [64] fp32): the convolution's weight gradient written into ``dw`` (shape of w,
    bf16 or fp32, any strides) and the BatchNorm parameter gradients, from dy [B, 64, T, F // 2]."""
    if not convfirst_applicable(x, w) or dw.shape != w.shape or dw.dtype not in (torch.float32, torch.bfloat16):
        raise SeldNativeError("convfirst: unsupported shapes, dtypes or layouts")
    b, _, t, f = x.shape
    if tuple(dy.shape) != (b, w.shape[0], t, f // 2):
        raise SeldNativeError("convfirst: dy does not match the block's output")
    if dy.dtype != x.dtype or not dy.is_contiguous(memory_format=torch.channels_last):
        dy = dy.to(x.dtype).contiguous(memory_format=torch.channels_last)
    index = ensure_init(x.device)
    dgb = torch.empty((2, w.shape[0]), dtype=torch.float32, device=x.device)
    lib = load_library()
    ws = torch.empty(int(lib.seld_convfirst_workspace_floats(1)), dtype=torch.float32, device=x.device)
    with _device_guard(index):
        check(lib.seld_convfirst_backward(_p(x), _p(w), _is_bf16(w), *w.stride(), _p(dy), b, t, f, _p(mean_invstd),
                                          _p(scale_shift), _p(dw), _is_bf16(dw), *dw.stride(), _p(dgb[0]), _p(dgb[1]),
                                          _p(ws), int(phases), _stream_ptr(x.device)), "seld_convfirst_backward")
    return dw, dgb[0], dgb[1]


# --------------------------------------------------------------------------- STFT / spatial features

def _prep_pcm(pcm):
    squeeze = pcm.dim() == 2
    if squeeze:
        pcm = pcm.unsqueeze(0)
    if pcm.dim() != 3 or not pcm.is_cuda or pcm.dtype not in (torch.float32, torch.int16):
        raise SeldNativeError("pcm must be a GPU tensor [N, C, L] (or [C, L]) of float32 or int16")
    return pcm.contiguous(), squeeze


def stft(pcm: torch.Tensor) -> torch.Tensor:
    """Complex STFT (960 / 480 / periodic Hann / center, reflect): [N, C, L] -> complex64 [N, C, F, 481]
    (frame-major; ``.transpose(-1, -2)`` gives torch.stft's [.., 481, F])."""
    pcm, squeeze = _prep_pcm(pcm)
    n, c, length = pcm.shape
    index = ensure_init(pcm.device)
    out = torch.empty((n, c, num_frames(length), N_BINS, 2), dtype=torch.float32, device=pcm.device)
    fn = load_library().seld_stft_f32 if pcm.dtype == torch.float32 else load_library().seld_stft_i16
    with _device_guard(index):
        check(fn(_p(pcm), n, c, length, _p(out), _stream_ptr(pcm.device)), "seld_stft")
    spec = torch.view_as_complex(out)
    return spec[0] if squeeze else spec


NIPD_MAX_TAPS = 48          # capacity of a band in the table (csrc/nipd.hip kNipdMaxTaps; the widest band has 44 bins)
_nipd_tables = {}


def _nipd_defaults(min_hz, max_hz, sound_speed):
    """The range and the speed of sound: what the caller gave, else the Config values."""
    if min_hz is None or max_hz is None or sound_speed is None:
        from config import Config
        min_hz = Config.NIPD_MIN_HZ if min_hz is None else min_hz
        max_hz = Config.NIPD_MAX_HZ if max_hz is None else max_hz
        sound_speed = Config.SOUND_SPEED if sound_speed is None else sound_speed
    return float(min_hz), float(max_hz), float(sound_speed)


def nipd_table_host(min_hz: float | None = None, max_hz: float | None = None, sound_speed: float | None = None):
    """The sparse mel-band NIPD weights on the host, no GPU needed: (first_bin int32 [64], taps int32
    [64], w float32 [64, 48], w_f64 float64 [64, 48]) as numpy arrays.  Raises for a range the library refuses."""
    import numpy as np
    min_hz, max_hz, sound_speed = _nipd_defaults(min_hz, max_hz, sound_speed)
    first, taps = np.zeros(N_MELS, dtype=np.int32), np.zeros(N_MELS, dtype=np.int32)
    w, w64 = np.zeros((N_MELS, NIPD_MAX_TAPS), dtype=np.float32), np.zeros((N_MELS, NIPD_MAX_TAPS), dtype=np.float64)
    check(load_library().seld_nipd_table_host(min_hz, max_hz, sound_speed, ctypes.c_void_p(first.ctypes.data),
                                              ctypes.c_void_p(taps.ctypes.data), ctypes.c_void_p(w.ctypes.data),
                                              ctypes.c_void_p(w64.ctypes.data)), "seld_nipd_table_host")
    return first, taps, w, w64


def nipd_pack_table(first_bin, taps, w) -> torch.Tensor:
    """The device table's layout as one int32 host tensor: first_bin[64] | taps[64] | the bits of w[64][48]."""
    import numpy as np
    packed = np.concatenate([np.asarray(first_bin, dtype=np.int32).reshape(N_MELS), np.asarray(taps, dtype=np.int32).reshape(N_MELS),
                             np.ascontiguousarray(w, dtype=np.float32).reshape(N_MELS * NIPD_MAX_TAPS).view(np.int32)])
    assert packed.nbytes == int(load_library().seld_nipd_table_bytes())
    return torch.from_numpy(packed)


def nipd_table(device, min_hz: float | None = None, max_hz: float | None = None, sound_speed: float | None = None):
    """(host tables as ``nipd_table_host``, device table int32 [3200]) of a range and speed, built once per device."""
    min_hz, max_hz, sound_speed = _nipd_defaults(min_hz, max_hz, sound_speed)
    device = torch.device(device)
    index = ensure_init(device)
    key = (index, min_hz, max_hz, sound_speed)
    hit = _nipd_tables.get(key)
    if hit is None:
        host = nipd_table_host(min_hz, max_hz, sound_speed)
        hit = (host, nipd_pack_table(*host[:3]).to(torch.device("cuda", index)))
        _nipd_tables[key] = hit
    return hit


def nipd_q15(phasors: torch.Tensor, out: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """csrc/nipd.hip on the words of ``seld_logmel_phasors_*``: phasors int32 [N, C, F, pitch] (2 <= C <= 8), ``table`` a
    device table (``nipd_table``), ``out`` float32 [N, F, C - 1, 64] -- any view with unit band stride and 16-byte aligned
    rows, e.g. channels C.. of a [N, F, 2C - 1, 64] feature tensor -- which receives nipd_1 .. nipd_{C-1}."""
    n, c, frames, pitch = phasors.shape
    if phasors.dtype != torch.int32 or not phasors.is_contiguous() or pitch != int(load_library().seld_phasor_pitch()):
        raise ValueError("nipd_q15: phasors must be contiguous int32 [N, C, F, seld_phasor_pitch()]")
    if out.dtype != torch.float32 or tuple(out.shape) != (n, frames, c - 1, N_MELS) or out.device != phasors.device:
        raise ValueError(f"nipd_q15: out must be float32 {(n, frames, c - 1, N_MELS)} on {phasors.device}")
    if table.dtype != torch.int32 or table.device != phasors.device or not table.is_contiguous() \
            or table.numel() * 4 != int(load_library().seld_nipd_table_bytes()):
        raise ValueError("nipd_q15: table must be the int32 device table of nipd_table()")
    index = ensure_init(phasors.device)
    s_n, s_t, s_c, s_m = out.stride()
    with _device_guard(index):
        check(load_library().seld_nipd_q15(_p(phasors), n, c, frames, _p(table), _p(out), s_n, s_c, s_m, s_t,
                                           _stream_ptr(phasors.device)), "seld_nipd_q15")
    return out


def feature_channels(kind: str, c: int) -> int:
    """Feature channels of ``spatial_features(pcm, kind)`` for ``c`` input channels; ValueError for a kind it does not
    know or a channel count the kind does not take."""
    if kind == "logmel":
        return c
    if kind == "logmel_iv":
        if c != 4:
            raise ValueError("FOA intensity vectors need 4 channels (W first)")
        return c + 3
    if kind == "logmel_gcc":
        if not 2 <= c <= 8:
            raise ValueError("GCC-PHAT supports 2..8 channels")
        return c + c * (c - 1) // 2
    if kind == "logmel_nipd":
        if not 2 <= c <= 8:
            raise ValueError("NIPD supports 2..8 channels")
        return c + c - 1
    raise ValueError(f"unknown feature kind {kind!r}")


def spatial_features(pcm: torch.Tensor, kind: str, nipd_min_hz: float | None = None, nipd_max_hz: float | None = None,
                     sound_speed: float | None = None) -> torch.Tensor:
    """Time-major feature tensor [N, F, C_total, 64] (float32) for one of
      'logmel'      C_total = C                       (the reference's features)
      'logmel_iv'   C_total = 4 + 3   (FOA: log-mel + mel-projected intensity vectors; needs C = 4)
      'logmel_gcc'  C_total = C + C(C-1)/2            (MIC: log-mel + GCC-PHAT, 2 <= C <= 8)
      'logmel_nipd' C_total = C + C - 1               (MIC: log-mel + mel-band NIPD against channel 0, 2 <= C <= 8; the
                    range and the speed of sound from the keyword arguments, else Config.NIPD_MIN_HZ / NIPD_MAX_HZ /
                    SOUND_SPEED)."""
    pcm, squeeze = _prep_pcm(pcm)
    n, c, length = pcm.shape
    frames = num_frames(length)
    if kind == "logmel":
        out = logmel(pcm, layout="tcf")
        return out[0] if squeeze else out
    index = ensure_init(pcm.device)
    total = feature_channels(kind, c)
    out = torch.empty((n, frames, total, N_MELS), dtype=torch.float32, device=pcm.device)
    s_n, s_t, s_c, s_m = frames * total * N_MELS, total * N_MELS, N_MELS, 1
    lib = load_library()
    stream = _stream_ptr(pcm.device)
    if kind == "logmel_nipd":
        # the phasor pass of 'logmel_gcc' (the same log-mel channels, bit for bit), then the NIPD kernel on its words
        _, table = nipd_table(pcm.device, nipd_min_hz, nipd_max_hz, sound_speed)
        pitch = int(lib.seld_phasor_pitch())
        with _device_guard(index):
            phasors = torch.empty((n, c, frames, pitch), dtype=torch.int32, device=pcm.device)
            fn = lib.seld_logmel_phasors_f32 if pcm.dtype == torch.float32 else lib.seld_logmel_phasors_i16
            check(fn(_p(pcm), n, c, length, _p(out), s_n, s_c, s_m, s_t, _p(phasors), stream), "seld_logmel_phasors")
        nipd_q15(phasors, out[:, :, c:], table)
        return out[0] if squeeze else out
    import os
    mode = os.environ.get("SELD_GCC", "mfma")                # developer A/B: "fft" = the FFT kernel, "spectra" = the
    if kind == "logmel_gcc" and mode not in ("fft", "spectra"):     # matrix-core kernel fed with complex64 spectra
        # ("planar" is read by the library: the Q15 kernel that unpacks the words to fp32 in LDS)
        # default: the log-mel pass also writes every bin's phasor X / |X| as Q15 pairs (4 B per bin instead of the 8 B of
        # the complex64 spectrum: half the HBM bytes on both sides) and the matrix-core GCC-PHAT kernel reads those
        pitch = int(lib.seld_phasor_pitch())
        with _device_guard(index):
            phasors = torch.empty((n, c, frames, pitch), dtype=torch.int32, device=pcm.device)
            fn = lib.seld_logmel_phasors_f32 if pcm.dtype == torch.float32 else lib.seld_logmel_phasors_i16
            check(fn(_p(pcm), n, c, length, _p(out), s_n, s_c, s_m, s_t, _p(phasors), stream), "seld_logmel_phasors")
            tail = ctypes.c_void_p(out.data_ptr() + c * N_MELS * 4)          # channel offset c
            check(lib.seld_gcc_phat_q15(_p(phasors), n, c, frames, tail, s_n, s_c, s_m, s_t, stream), "seld_gcc_phat_q15")
        return out[0] if squeeze else out
    if kind == "logmel_iv" and os.environ.get("SELD_FOA", "fused") != "spectra":
        # default: ONE kernel -- the four channels of a clip meet in one workgroup, the spectra stay in LDS
        # (csrc/logmel.hip logmel_iv_kernel; SELD_FOA=spectra: the two-kernel form through complex64 spectra, developer A/B)
        fn = lib.seld_logmel_iv_f32 if pcm.dtype == torch.float32 else lib.seld_logmel_iv_i16
        with _device_guard(index):
            check(fn(_p(pcm), n, length, _p(out), s_n, s_c, s_m, s_t, stream), "seld_logmel_iv")
        return out[0] if squeeze else out
    with _device_guard(index):
        # one pass over the PCM: the log-mel channels and the spectra the spatial kernels read
        spec = torch.empty((n, c, frames, N_FFT // 2 + 1, 2), dtype=torch.float32, device=pcm.device)
        fn = lib.seld_logmel_spectrum_f32 if pcm.dtype == torch.float32 else lib.seld_logmel_spectrum_i16
        check(fn(_p(pcm), n, c, length, _p(out), s_n, s_c, s_m, s_t, _p(spec), stream), "seld_logmel_spectrum")
        tail = ctypes.c_void_p(out.data_ptr() + c * N_MELS * 4)              # channel offset c
        if kind == "logmel_iv":
            check(lib.seld_foa_intensity(_p(spec), n, frames, tail, s_n, s_c, s_m, s_t, stream), "seld_foa_intensity")
        else:
            check(lib.seld_gcc_phat(_p(spec), n, c, frames, tail, s_n, s_c, s_m, s_t, stream), "seld_gcc_phat")
    return out[0] if squeeze else out
