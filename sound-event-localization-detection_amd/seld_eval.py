"""SELD evaluation: the model's spatial grid maps -> DOA events, and the location-aware metrics F20 / ER20 / LE_CD / LR_CD.

The reference has no such code (its test_model, trainer.py:394-711, reports argmax accuracy per grid cell); the
definitions are this project's, DESIGN.md section 10.  The hot paths are two HIP kernels (csrc/seld_eval.hip):

  seld_grid_decode   one streaming pass over the logits: softmax per cell, mean over the overlapping windows and over
                     the frames of each 100 ms meta-frame, 3x3 peak test per class, top-K per (meta-frame, class)
  seld_doa_match     per (meta-frame, class): minimum-cost assignment and maximum matching within the DOA threshold

Test-time augmentation (csrc/seld_tta.hip): ``patterns`` on decode / evaluate_logits switches to

  seld_grid_decode_tta   the same pass over one stack of logits per spatial pattern, each un-permuted to the original
                         frame as it is read, averaged before the peak test

Track linking (csrc/seld_track.hip): ``track`` on evaluate_logits puts between decode and match

  seld_track_link        one wavefront per (segment, class) links the frame-wise peaks into tracks with an identity over
                         time: gated greedy nearest-cell linking, gap filling, a minimum duration, onset / offset

Sub-cell DOA refinement (csrc/seld_refine.hip): ``refine`` on decode / evaluate_logits switches to

  seld_grid_decode_refine  either decode with an epilogue that gives every detection a direction finer than its cell,
                           from the peak's 3x3 neighbourhood of the class map while it is still in LDS
  seld_doa_match_dirs      seld_doa_match on those float directions

Threshold sweep and per-class thresholds (csrc/seld_sweep.hip): ``sweep`` / ``class_thresholds`` on
evaluate_logits decode once at the lowest threshold involved -- the detections at a higher one are a prefix -- and run

  seld_doa_match_prefix    seld_doa_match / seld_doa_match_dirs for every prefix of every (meta-frame, class) at once
  seld_sweep_score         the sums behind the metrics for up to 64 thresholds from those tables, one lane per threshold

Segment-based, class-macro metrics with jackknife intervals (csrc/seld_segment.hip): ``segment`` /
``jackknife`` on evaluate_logits add the figures published SELD results are given in, from

  seld_doa_assign          the assignment behind seld_doa_match's cost: per reference the distance to its detection
  seld_segment_score       the counts of every (1 s block, class), folded per recording
  seld_jackknife_score     micro and macro F / ER / LE / LR / SELD of every leave-one-recording-out replicate

The host side here builds the tables (meta-frames, reference CSR), drives the decode batch by batch as the windows are
computed, reduces the match counts on the device and writes event CSVs.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import functools
import math
from collections import namedtuple
from pathlib import Path

import numpy as np
import torch

from seld_native import SeldNativeError, _device_guard, _p, _stream_ptr, check, ensure_init, load_library

WIN = 250                  # frames per window (config.WINDOW_LENGTH / SPECTROGRAM_HOP_LENGTH)
HOP = 50                   # frames between window starts (config.HOP_LENGTH / SPECTROGRAM_HOP_LENGTH)
FRAMES_PER_META = 5        # 100 ms meta-frame / 20 ms label frame (dataset.py:100-103)
NUM_EVENT_CLASSES = 13     # class 13 is the background
GRID_I, GRID_J = 18, 36
MAX_PEAKS = 8              # K limit of the decode kernel
MAX_REFS = 8               # references per (meta-frame, class) the match kernel enumerates
DOA_MARGIN_DEG = 1e-6      # a pair counts within the threshold when d <= threshold + 1e-6 degrees
# Windows kept from one decode call to the next.  A meta-frame needs every window that covers one of its frames: up to
# five per frame, and six when its frames straddle a window start (frames 50 k - 1 and 50 k).  Its last covering window
# is in the current batch, so the five before the batch are enough.
KEEP_WINDOWS = 5


# ------------------------------------------------------------------------------------------------------ meta-frames

class MetaFrameTable:
    """Every meta-frame of a timeline, in timeline order.  Host arrays (int64 unless noted), length Q:
    ``first`` global first frame, ``length`` frame count (int32, 1..5), ``segment`` segment index (int32), ``index`` the
    meta-frame number m within its segment, ``first_window`` / ``last_window`` the windows covering its first / last
    frame; ``seg_offsets`` [S + 1]: the meta-frames of segment s are ``seg_offsets[s]:seg_offsets[s + 1]``.
    ``total`` frames on the timeline, ``windows`` = ceil(total / 50)."""

    def __init__(self, segments, total=None):
        seg = np.asarray(segments, dtype=np.int64).reshape(-1, 2)
        if (seg < 0).any():
            raise ValueError("segments must be (first_frame >= 0, n_frames >= 0)")
        counts = (seg[:, 1] + FRAMES_PER_META - 1) // FRAMES_PER_META          # ceil(n / 5) meta-frames per segment
        self.seg_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.segment = np.repeat(np.arange(len(seg), dtype=np.int32), counts)
        self.index = np.arange(int(self.seg_offsets[-1]), dtype=np.int64) - self.seg_offsets[:-1][self.segment]
        starts = FRAMES_PER_META * self.index
        self.first = seg[self.segment, 0] + starts
        self.length = np.minimum(FRAMES_PER_META, seg[self.segment, 1] - starts).astype(np.int32)
        self.segments = seg
        end = int((seg[:, 0] + seg[:, 1]).max()) if len(seg) else 0
        self.total = end if total is None else int(total)
        if self.total < end:
            raise ValueError(f"segments reach frame {end}, beyond the timeline's {self.total}")
        self.windows = (self.total + HOP - 1) // HOP
        last = self.first + self.length - 1
        self.first_window = np.where(self.first < WIN, 0, (self.first - WIN) // HOP + 1)
        self.last_window = np.minimum(last // HOP, self.windows - 1)
        if (np.diff(self.last_window) < 0).any():
            raise ValueError("segments must be in timeline order")
        self._device = {}

    def __len__(self):
        return int(self.first.shape[0])

    def device(self, device):
        """(first int64 [Q], length int32 [Q]) on ``device``, uploaded once."""
        key = str(device)
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.first.copy()).to(device),
                                 torch.from_numpy(self.length.copy()).to(device))
        return self._device[key]

    def device_segments(self, device):
        """(seg_offsets int64 [S + 1], segment int64 [Q]) on ``device``, uploaded once."""
        key = ("segments", str(device))
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.seg_offsets.astype(np.int64)).to(device),
                                 torch.from_numpy(self.segment.astype(np.int64)).to(device))
        return self._device[key]


def meta_frame_table(segments, total=None) -> MetaFrameTable:
    """Segments (first_frame, n_frames) int [S, 2] -> the timeline's meta-frames: meta-frame m of segment s covers frames
    first + 5m .. first + min(5m + 5, n) - 1, m < ceil(n / 5) (the label rule of dataset.py:100-103)."""
    return MetaFrameTable(segments, total)


# ------------------------------------------------------------------------------------------------------ kernels

def _grid_decode(name, logits, patterns, refine, w0, table, q0, nq, threshold, max_peaks, out, probs):
    """The three decode wrappers: validation, the coverage check, the outputs and the one library call of the mode.
    ``patterns`` None: the plain walk over logits [nw, 250, 648, 14]; else one stack per pattern, [P, nw, 250, 648, 14].
    ``refine``: seld_grid_decode_refine (either walk) and a fourth output, det_dir; else seld_grid_decode[_tta]."""
    stacked = patterns is not None
    pats = np.asarray(list(patterns) if stacked else [], dtype=np.int32).reshape(-1)
    if not logits.is_cuda:
        raise SeldNativeError(f"{name}: logits must live on the GPU (no CPU fallback)")
    if logits.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"{name}: logits must be bfloat16 or float32")
    if logits.dim() != (5 if stacked else 4) or \
            tuple(logits.shape[-3:]) != (WIN, GRID_I * GRID_J, NUM_EVENT_CLASSES + 1):
        raise ValueError(f"{name}: logits must be {'[P, nw' if stacked else '[nw'}, {WIN}, 648, 14], got "
                         f"{tuple(logits.shape)}")
    if stacked and int(logits.shape[0]) != len(pats):
        raise ValueError(f"{name}: {int(logits.shape[0])} stacks of logits for {len(pats)} patterns")
    logits = logits.contiguous()
    nw = int(logits.shape[-4])
    if not (q0 >= 0 and nq >= 0 and q0 + nq <= len(table)):
        raise ValueError(f"{name}: meta-frame range outside the table")
    if nq:
        lo, hi = int(table.first_window[q0:q0 + nq].min()), int(table.last_window[q0:q0 + nq].max())
        if lo < w0 or hi >= w0 + nw:
            raise SeldNativeError(f"{name}: meta-frames {q0}..{q0 + nq - 1} need windows {lo}..{hi}, the call "
                                  f"holds {w0}..{w0 + nw - 1}")
    device = logits.device
    index = ensure_init(device)
    k = int(max_peaks)
    if out is None:
        out = (torch.empty((nq, NUM_EVENT_CLASSES, max(k, 1)), dtype=torch.int32, device=device),
               torch.empty((nq, NUM_EVENT_CLASSES, max(k, 1)), dtype=torch.float32, device=device),
               torch.empty((nq, NUM_EVENT_CLASSES), dtype=torch.int32, device=device))
        if refine:
            out += (torch.empty((nq, NUM_EVENT_CLASSES, max(k, 1), 2), dtype=torch.float32, device=device),)
    first, length = table.device(device)
    lib = load_library()
    head = (_p(logits), int(logits.dtype == torch.bfloat16), int(w0), nw, table.windows, table.total, _p(first),
            _p(length), int(q0), int(nq))
    pat = (pats.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if stacked else None, len(pats))
    tail = (float(threshold), k) + ((_p(cell_unit_table(device)),) if refine else ()) + tuple(_p(t) for t in out) + \
        (_p(probs), _stream_ptr(device))
    with _device_guard(index):
        if refine:
            rc = lib.seld_grid_decode_refine(*head, *pat, *tail)
        elif stacked:
            rc = lib.seld_grid_decode_tta(*head, *pat, *tail)
        else:
            rc = lib.seld_grid_decode(*head, *tail)
        check(rc, "seld_" + name)
    return out


def grid_decode(logits: torch.Tensor, w0: int, table: MetaFrameTable, q0: int, nq: int, threshold: float, max_peaks: int,
                out=None, probs: torch.Tensor | None = None):
    """seld_grid_decode over meta-frames [q0, q0 + nq) from ``logits`` [nw, 250, 648, 14] (bf16 or fp32, GPU) holding
    windows [w0, w0 + nw).  ``out``: contiguous (det_cell int32 [nq, 13, K], det_score f32 [nq, 13, K], det_count int32
    [nq, 13]) to write, else allocated.  ``probs``: f32 [nq, 648, 13] to receive P_q, or None.
    Raises SeldNativeError, launching nothing, when a window that covers one of the meta-frames is not in ``logits``."""
    return _grid_decode("grid_decode", logits, None, False, w0, table, q0, nq, threshold, max_peaks, out, probs)


def grid_decode_tta(logits: torch.Tensor, patterns, w0: int, table: MetaFrameTable, q0: int, nq: int, threshold: float,
                    max_peaks: int, out=None, probs: torch.Tensor | None = None):
    """seld_grid_decode_tta: ``grid_decode`` over ``logits`` [P, nw, 250, 648, 14], stack n holding windows
    [w0, w0 + nw) gathered with spatial pattern ``patterns[n]``; the stacks are averaged in the original frame
    (DESIGN.md section 13).  ``out`` / ``probs`` and the coverage check as ``grid_decode``; the pattern list itself is
    checked by the library (SeldNativeError)."""
    return _grid_decode("grid_decode_tta", logits, list(patterns), False, w0, table, q0, nq, threshold, max_peaks, out,
                        probs)


def _match_inputs(name, det_cell, det_dir, det_count, ref_offsets, ref_dirs):
    """The prologue of the four matching wrappers.  The detections are ``det_dir`` f32 [Q, 13, K, 2] when given, else
    ``det_cell`` int32 [Q, 13, K], with det_count [Q, 13] and ref_offsets of Q * 13 + 1 entries.  Returns (device index,
    device, Q, K, det_cell or None, det_dir or None, det_count, ref_offsets, ref_dirs), the tensors cast and contiguous;
    an empty ``ref_dirs`` is replaced by one row that nothing reads."""
    dets, shape = (det_cell, "det_cell must be [Q, 13, K]") if det_dir is None else (det_dir, "det_dir must be [Q, 13, K, 2]")
    if not (dets.is_cuda and det_count.is_cuda):
        raise SeldNativeError(f"{name}: detections must live on the GPU (no CPU fallback)")
    if dets.dim() != (3 if det_dir is None else 4) or dets.shape[1] != NUM_EVENT_CLASSES or \
            (det_dir is not None and dets.shape[3] != 2) or tuple(det_count.shape) != tuple(dets.shape[:2]):
        raise ValueError(f"{name}: {shape} and det_count [Q, 13]")
    q, k, device = int(dets.shape[0]), int(dets.shape[2]), dets.device
    if ref_offsets.numel() != q * NUM_EVENT_CLASSES + 1:
        raise ValueError(f"{name}: ref_offsets must have Q * 13 + 1 entries")
    index = ensure_init(device)
    dirs = ref_dirs if ref_dirs.numel() else torch.zeros((1, 2), dtype=torch.int32, device=device)
    dets = dets.to(torch.int32 if det_dir is None else torch.float32).contiguous()
    return (index, device, q, k, dets if det_dir is None else None, None if det_dir is None else dets,
            det_count.to(torch.int32).contiguous(), ref_offsets.to(torch.int32).contiguous(),
            dirs.to(torch.int32).contiguous())


def doa_match(det_cell: torch.Tensor, det_count: torch.Tensor, ref_offsets: torch.Tensor, ref_dirs: torch.Tensor,
              doa_threshold_deg: float, I: int = GRID_I, J: int = GRID_J):
    """seld_doa_match: (stats int32 [Q, 13, 4] = (R, P, k, tp), cost f64 [Q, 13]) on the detections' device.  A pair is
    within the threshold when d <= doa_threshold_deg + DOA_MARGIN_DEG."""
    index, device, q, k, det_cell, _, det_count, ref_offsets, dirs = _match_inputs("doa_match", det_cell, None, det_count,
                                                                                   ref_offsets, ref_dirs)
    stats = torch.empty((q, NUM_EVENT_CLASSES, 4), dtype=torch.int32, device=device)
    cost = torch.empty((q, NUM_EVENT_CLASSES), dtype=torch.float64, device=device)
    with _device_guard(index):
        check(load_library().seld_doa_match(_p(det_cell), _p(det_count), k, _p(ref_offsets), _p(dirs), q, int(I), int(J),
                                            float(doa_threshold_deg) + DOA_MARGIN_DEG, _p(stats), _p(cost),
                                            _stream_ptr(device)), "seld_doa_match")
    return stats, cost


# ------------------------------------------------------------------------------------------------------ refinement

_cell_units = {}


def cell_unit_table(device=None, I: int = GRID_I, J: int = GRID_J) -> torch.Tensor:
    """The unit vectors of the cell centres, f32 [I * J, 3] = (cos el cos az, cos el sin az, sin el): computed in float64,
    rounded once to fp32, cached per device (``device`` None: the host copy).  The table seld_grid_decode_refine reads."""
    host_key, key = (int(I), int(J), None), (int(I), int(J), None if device is None else str(device))
    if host_key not in _cell_units:
        cell = np.arange(int(I) * int(J), dtype=np.int64)
        az = np.deg2rad(-180.0 + (cell % J + 0.5) * (360.0 / J))
        el = np.deg2rad(-90.0 + (cell // J + 0.5) * (180.0 / I))
        unit = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
        _cell_units[host_key] = torch.from_numpy(unit.astype(np.float32))
    if key not in _cell_units:
        _cell_units[key] = _cell_units[host_key].to(device).contiguous()
    return _cell_units[key]


def grid_decode_refine(logits: torch.Tensor, w0: int, table: MetaFrameTable, q0: int, nq: int, threshold: float,
                       max_peaks: int, out=None, probs: torch.Tensor | None = None, patterns=None):
    """seld_grid_decode_refine: ``grid_decode`` (``patterns`` None or empty; logits [nw, 250, 648, 14]) or
    ``grid_decode_tta`` (logits [P, nw, 250, 648, 14]) that also writes every detection's sub-cell direction (DESIGN.md
    section 15).  ``out``: contiguous (det_cell, det_score, det_count, det_dir f32 [nq, 13, K, 2] = (az, el) degrees, 0
    past the count) to write, else allocated; the first three and ``probs`` are the un-refined call's bit for bit."""
    patterns = list(patterns) if patterns is not None else []
    return _grid_decode("grid_decode_refine", logits, patterns or None, True, w0, table, q0, nq, threshold, max_peaks, out,
                        probs)


def doa_match_dirs(det_dir: torch.Tensor, det_count: torch.Tensor, ref_offsets: torch.Tensor, ref_dirs: torch.Tensor,
                   doa_threshold_deg: float):
    """seld_doa_match_dirs: ``doa_match`` with the detections' directions det_dir f32 [Q, 13, K, 2] = (az, el) degrees in
    place of their cells."""
    index, device, q, k, _, det_dir, det_count, ref_offsets, dirs = _match_inputs("doa_match_dirs", None, det_dir,
                                                                                  det_count, ref_offsets, ref_dirs)
    stats = torch.empty((q, NUM_EVENT_CLASSES, 4), dtype=torch.int32, device=device)
    cost = torch.empty((q, NUM_EVENT_CLASSES), dtype=torch.float64, device=device)
    with _device_guard(index):
        check(load_library().seld_doa_match_dirs(_p(det_dir), _p(det_count), k, _p(ref_offsets), _p(dirs), q,
                                                 float(doa_threshold_deg) + DOA_MARGIN_DEG, _p(stats), _p(cost),
                                                 _stream_ptr(device)), "seld_doa_match_dirs")
    return stats, cost


def cell_centre_dirs(cells: torch.Tensor, I: int = GRID_I, J: int = GRID_J) -> torch.Tensor:
    """Cells int [...] -> their centres f32 [..., 2] = (az, el) degrees (exact in fp32 on the 10-degree grid)."""
    cells = cells.to(torch.int64)
    az = -180.0 + (cells % J).to(torch.float32).add(0.5) * (360.0 / J)
    el = -90.0 + torch.div(cells, J, rounding_mode="floor").to(torch.float32).add(0.5) * (180.0 / I)
    return torch.stack([az, el], dim=-1)


def track_dirs(trk_cell: torch.Tensor, trk_count: torch.Tensor, det_cell: torch.Tensor, det_count: torch.Tensor,
               det_dir: torch.Tensor, I: int = GRID_I, J: int = GRID_J) -> torch.Tensor:
    """Directions of ``track``'s surviving emissions, f32 [Q, 13, 8, 2]: an emission takes the refined direction of the
    detection with the same cell at its (q, c) (a frame's detections of one class are distinct cells); a gap-filled
    emission, whose cell is not among that frame's detections, takes its cell centre; 0 past trk_count.  Framework ops
    where the tensors live."""
    k = int(det_cell.shape[-1])
    rank = torch.arange(k, device=det_cell.device)
    valid = rank < det_count[..., None]                                             # [Q, 13, K]
    same = (trk_cell[..., :, None] == det_cell[..., None, :]) & valid[..., None, :]  # [Q, 13, 8, K]
    found = same.any(-1)
    pick = same.to(torch.int32).argmax(-1)                                           # the detection's rank, 0 when none
    taken = torch.gather(det_dir, 2, pick[..., None].expand(-1, -1, -1, 2))
    dirs = torch.where(found[..., None], taken, cell_centre_dirs(trk_cell, I, J))
    slot = torch.arange(int(trk_cell.shape[-1]), device=trk_cell.device)
    return torch.where((slot < trk_count[..., None])[..., None], dirs, torch.zeros_like(dirs))


# ------------------------------------------------------------------------------------------------------ tracking

_distance_tables = {}


def _distance_table_host(I: int, J: int) -> np.ndarray:
    """int32 [I, I, J]: rint(1000 d), d the float64 great-circle angle in degrees between the centres of cells (i_a, j_a)
    and (i_b, j_b) by the atan2 form of DESIGN.md 10.1, indexed (i_a, i_b, (j_b - j_a) mod J)."""
    rad = np.pi / 180.0
    el = (-90.0 + (np.arange(I, dtype=np.float64) + 0.5) * (180.0 / I)) * rad
    az = (np.arange(J, dtype=np.float64) * (360.0 / J)) * rad             # j_b - j_a cells of azimuth
    e1, e2, a2 = np.broadcast_arrays(el[:, None, None], el[None, :, None], az[None, None, :])
    u = np.stack([np.cos(e1), np.zeros_like(e1), np.sin(e1)], -1)
    v = np.stack([np.cos(e2) * np.cos(a2), np.cos(e2) * np.sin(a2), np.sin(e2)], -1)
    cr = np.cross(u, v)
    d = np.arctan2(np.sqrt((cr ** 2).sum(-1)), (u * v).sum(-1)) * (180.0 / np.pi)
    d[np.arange(I), np.arange(I), 0] = 0.0                                 # identical cells are exactly 0
    return np.rint(1000.0 * d).astype(np.int32)


def track_distance_table(I: int = GRID_I, J: int = GRID_J, device=None) -> torch.Tensor:
    """The cell-to-cell distance table of the track kernel in milli-degrees, int32 [I, I, J]; built once with numpy and
    cached per device (``device`` None: the host copy)."""
    host_key, key = (int(I), int(J), None), (int(I), int(J), None if device is None else str(device))
    if host_key not in _distance_tables:
        _distance_tables[host_key] = torch.from_numpy(_distance_table_host(int(I), int(J)))
    if key not in _distance_tables:
        _distance_tables[key] = _distance_tables[host_key].to(device)
    return _distance_tables[key]


def track_settings(track) -> dict | None:
    """``track`` as evaluate_logits takes it -> {gate_deg, max_gap, min_len} or None (off).  None reads Config.SELD_TRACK;
    True or a dict switches tracking on, a dict's keys override the Config.SELD_TRACK_* defaults."""
    from config import Config
    if track is None:
        track = bool(getattr(Config, "SELD_TRACK", False))
    if track is False:
        return None
    settings = {"gate_deg": float(Config.SELD_TRACK_GATE_DEG), "max_gap": int(Config.SELD_TRACK_MAX_GAP),
                "min_len": int(Config.SELD_TRACK_MIN_LEN)}
    if isinstance(track, dict):
        unknown = set(track) - set(settings)
        if unknown:
            raise ValueError(f"track: unknown keys {sorted(unknown)}; expected gate_deg, max_gap, min_len")
        settings.update(gate_deg=float(track.get("gate_deg", settings["gate_deg"])),
                        max_gap=int(track.get("max_gap", settings["max_gap"])),
                        min_len=int(track.get("min_len", settings["min_len"])))
    elif track is not True:
        raise TypeError("track must be None, a bool or a dict")
    return settings


def track(det_cell: torch.Tensor, det_count: torch.Tensor, table: MetaFrameTable, gate_deg: float, max_gap: int,
          min_len: int, I: int = GRID_I, J: int = GRID_J):
    """seld_track_link: the decode's outputs det_cell int32 [Q, 13, K] / det_count int32 [Q, 13] of
    the timeline of ``table`` -> (trk_cell int32 [Q, 13, 8], trk_id int32 [Q, 13, 8], trk_count int32 [Q, 13], tracks
    int32 [T, 4] = (first_m, last_m, detected, kept), chain_tracks int32 [13 S], chain_offsets int64 [13 S + 1]) on the
    detections' device.  Track ``id`` of chain x = 13 s + c is row chain_offsets[x] + id; rows no track uses are 0."""
    if not (det_cell.is_cuda and det_count.is_cuda):
        raise SeldNativeError("track: detections must live on the GPU (no CPU fallback)")
    if det_cell.dim() != 3 or det_cell.shape[1] != NUM_EVENT_CLASSES or tuple(det_count.shape) != tuple(det_cell.shape[:2]):
        raise ValueError("track: det_cell must be [Q, 13, K] and det_count [Q, 13]")
    q, k = int(det_cell.shape[0]), int(det_cell.shape[2])
    if q != len(table):
        raise ValueError(f"track: {q} meta-frames of detections for a timeline of {len(table)}")
    device = det_cell.device
    index = ensure_init(device)
    gate_mdeg = int(np.rint(1000.0 * float(gate_deg)))
    det_cell, det_count = det_cell.to(torch.int32).contiguous(), det_count.to(torch.int32).contiguous()
    n_seg = len(table.seg_offsets) - 1
    seg_offsets, segment = table.device_segments(device)
    # detections per chain (segment, class): an integer index_add over the meta-frames (a scan along the timeline costs
    # four times the track kernels)
    per_chain = torch.zeros((n_seg, NUM_EVENT_CLASSES), dtype=torch.int64, device=device)
    per_chain.index_add_(0, segment, det_count.clamp(0, max(k, 0)).to(torch.int64))
    per_chain = per_chain.reshape(-1)
    chain_offsets = torch.zeros(n_seg * NUM_EVENT_CLASSES + 1, dtype=torch.int64, device=device)
    chain_offsets[1:] = torch.cumsum(per_chain, 0)
    rank = torch.arange(k, dtype=torch.int32, device=device)
    stray = ((det_cell < 0) | (det_cell >= int(I) * int(J))) & (rank < det_count[..., None])
    total, stray = (int(v) for v in torch.stack([chain_offsets[-1], stray.sum()]).tolist())    # the one host read
    if stray:
        raise ValueError(f"track: {stray} detections lie outside the {I} x {J} grid")
    trk_cell = torch.empty((q, NUM_EVENT_CLASSES, MAX_PEAKS), dtype=torch.int32, device=device)
    trk_id = torch.empty((q, NUM_EVENT_CLASSES, MAX_PEAKS), dtype=torch.int32, device=device)
    trk_count = torch.empty((q, NUM_EVENT_CLASSES), dtype=torch.int32, device=device)
    tracks = torch.zeros((max(total, 1), 4), dtype=torch.int32, device=device)
    chain_tracks = torch.zeros(max(n_seg * NUM_EVENT_CLASSES, 1), dtype=torch.int32, device=device)
    dist = track_distance_table(I, J, device)
    if q == 0:                                              # an empty timeline: nothing to launch
        return trk_cell, trk_id, trk_count, tracks[:0], chain_tracks[:n_seg * NUM_EVENT_CLASSES], chain_offsets
    with _device_guard(index):
        check(load_library().seld_track_link(_p(det_cell), _p(det_count), k, _p(seg_offsets), n_seg, _p(dist), int(I),
                                             int(J), gate_mdeg, int(max_gap), int(min_len), _p(chain_offsets),
                                             _p(trk_cell), _p(trk_id), _p(trk_count), _p(tracks), _p(chain_tracks),
                                             _stream_ptr(device)), "seld_track_link")
    return trk_cell, trk_id, trk_count, tracks[:total], chain_tracks[:n_seg * NUM_EVENT_CLASSES], chain_offsets


_track_link = track        # (evaluate_logits has a parameter of that name)


def track_summary(trk_count: torch.Tensor, tracks: torch.Tensor, chain_tracks: torch.Tensor) -> dict:
    """Counts of one ``track`` call, reduced on the device: tracks born, tracks kept, removed (shorter than min_len) and
    filled = emissions of kept tracks at frames where they were not detected."""
    t = tracks.to(torch.int64)
    sums = torch.stack([chain_tracks.to(torch.int64).sum(), t[:, 3].sum(), (t[:, 2] * t[:, 3]).sum(),
                        trk_count.to(torch.int64).sum()]).cpu().tolist()
    born, kept, detected, emitted = (int(v) for v in sums)
    return {"tracks": born, "tracks_kept": kept, "filled": emitted - detected, "removed": born - kept}


# ------------------------------------------------------------------------------------------------------ decode driver

def decode(batches, table: MetaFrameTable, threshold: float, max_peaks: int, device=None, keep_probs: bool = False,
           patterns=None, refine: bool = False):
    """Streaming decode of a whole timeline.  ``batches`` yields logit tensors [B, 250, 648, 14] of consecutive windows
    in timeline order (window 0 first, ``table.windows`` in all).  After each batch every meta-frame whose last
    covering window has been seen is decoded; the last KEEP_WINDOWS windows stay on the device for the next call.
    Returns (det_cell int32 [Q, 13, K], det_score f32 [Q, 13, K], det_count int32 [Q, 13], probs f32 [Q, 648, 13] or
    None) on the device.
    ``patterns``: a non-empty list of spatial patterns switches to test-time augmentation: the batches are then
    [P, B, 250, 648, 14], stack n under ``patterns[n]``, and every call goes to ``grid_decode_tta``.
    ``refine``: every call goes to ``grid_decode_refine`` (either walk) and a fifth tensor is returned: det_dir f32
    [Q, 13, K, 2], the detections' sub-cell directions."""
    k = int(max_peaks)
    patterns = tuple(patterns) if patterns is not None else ()
    wdim = 1 if patterns else 0                  # the window axis of a batch
    if not 1 <= k <= MAX_PEAKS:
        raise ValueError(f"max_peaks must be in 1..{MAX_PEAKS}, got {max_peaks}")
    n_q = len(table)
    det = probs = carry = None
    seen = 0                    # windows received so far
    done = 0                    # meta-frames decoded so far
    for batch in batches:
        if device is None:
            device = batch.device
        if det is None:
            det = (torch.empty((n_q, NUM_EVENT_CLASSES, k), dtype=torch.int32, device=device),
                   torch.empty((n_q, NUM_EVENT_CLASSES, k), dtype=torch.float32, device=device),
                   torch.empty((n_q, NUM_EVENT_CLASSES), dtype=torch.int32, device=device))
            if refine:
                det += (torch.empty((n_q, NUM_EVENT_CLASSES, k, 2), dtype=torch.float32, device=device),)
            if keep_probs:
                probs = torch.empty((n_q, GRID_I * GRID_J, NUM_EVENT_CLASSES), dtype=torch.float32, device=device)
        if batch.dtype not in (torch.bfloat16, torch.float32):
            batch = batch.float()
        held = batch if carry is None else torch.cat([carry, batch.to(carry.dtype)], dim=wdim)
        w0 = seen - (0 if carry is None else int(carry.shape[wdim]))
        seen += int(batch.shape[wdim])
        end = int(np.searchsorted(table.last_window, seen - 1, side="right"))
        if end > done:
            out = tuple(t[done:end] for t in det)
            if refine:
                grid_decode_refine(held, w0, table, done, end - done, threshold, k, out=out,
                                   probs=probs[done:end] if probs is not None else None, patterns=patterns)
            elif patterns:
                grid_decode_tta(held, patterns, w0, table, done, end - done, threshold, k, out=out,
                                probs=probs[done:end] if probs is not None else None)
            else:
                grid_decode(held, w0, table, done, end - done, threshold, k, out=out,
                            probs=probs[done:end] if probs is not None else None)
            done = end
        if patterns:            # (a producer may reuse its [P, B, ...] buffer: the first carry is still a view of the batch)
            carry = held[:, -KEEP_WINDOWS:].clone() if held is batch else held[:, -KEEP_WINDOWS:]
        else:
            carry = held[-KEEP_WINDOWS:]
    if seen != table.windows or done != n_q:
        raise ValueError(f"decode: the timeline has {table.windows} windows, got {seen}")
    if det is None:             # an empty timeline
        device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        det = (torch.zeros((0, NUM_EVENT_CLASSES, k), dtype=torch.int32, device=device),
               torch.zeros((0, NUM_EVENT_CLASSES, k), dtype=torch.float32, device=device),
               torch.zeros((0, NUM_EVENT_CLASSES), dtype=torch.int32, device=device))
        if refine:
            det += (torch.zeros((0, NUM_EVENT_CLASSES, k, 2), dtype=torch.float32, device=device),)
    return (det[0], det[1], det[2], probs, det[3]) if refine else (det[0], det[1], det[2], probs)


# ------------------------------------------------------------------------------------------------------ references

def reference_table(table: MetaFrameTable, metadata_rows):
    """CSR of the references per (meta-frame, class): (offsets int32 [Q * 13 + 1], dirs int32 [R, 2] = (az, el)).
    Rows of segment s with meta-frame m and class c < 13 land at q = seg_offsets[s] + m; rows with 5 m >= n (outside the
    cropped segment, as the rasteriser drops them) or negative m are dropped; rows keep their file order inside a (q, c).
    Raises ValueError when a (q, c) has more than MAX_REFS references."""
    keys, dirs = [np.zeros(0, np.int64)], [np.zeros((0, 2), np.int64)]
    for s, rows in enumerate(metadata_rows):
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5) if len(rows) else np.zeros((0, 5), np.int64)
        n = int(table.segments[s, 1])
        m, c = rows[:, 0], rows[:, 1]
        rows = rows[(m >= 0) & (FRAMES_PER_META * m < n) & (c >= 0) & (c < NUM_EVENT_CLASSES)]
        keys.append((table.seg_offsets[s] + rows[:, 0]) * NUM_EVENT_CLASSES + rows[:, 1])
        dirs.append(rows[:, 3:5])
    n_qc = len(table) * NUM_EVENT_CLASSES
    key, dirs = np.concatenate(keys), np.concatenate(dirs)
    counts = np.bincount(key, minlength=n_qc)
    if counts.size and counts.max() > MAX_REFS:
        bad = int(np.argmax(counts))
        raise ValueError(f"meta-frame {bad // NUM_EVENT_CLASSES}, class {bad % NUM_EVENT_CLASSES} has {int(counts.max())} "
                         f"references; the matcher takes at most {MAX_REFS}")
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    order = np.argsort(key, kind="stable")
    return offsets, np.ascontiguousarray(dirs[order].astype(np.int32)).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------------ metrics

def score(stats: torch.Tensor, cost: torch.Tensor) -> dict:
    """Micro-averaged metrics from the per-(q, c) match results: stats int [Q, 13, 4] = (R, P, k, tp), cost float [Q, 13].
    Counts are reduced in int64 and the cost in float64 where the tensors live; only the totals and the per-class
    vectors are copied to the host.  Empty denominators give nan."""
    st = stats.to(torch.int64)
    r, p, k, tp = st[..., 0], st[..., 1], st[..., 2], st[..., 3]
    fn_qc, fp_qc = r - tp, p - tp
    fn_q, fp_q = fn_qc.sum(1), fp_qc.sum(1)
    totals = torch.stack([torch.minimum(fn_q, fp_q).sum(), torch.clamp(fn_q - fp_q, min=0).sum(),
                          torch.clamp(fp_q - fn_q, min=0).sum()])                                  # S, D, I
    counts = torch.stack([tp.sum(0), fp_qc.sum(0), fn_qc.sum(0), r.sum(0), k.sum(0)])            # [5, 13]
    cost_c = cost.to(torch.float64).sum(0)
    return _score_record(counts.cpu().numpy(), totals.cpu().numpy(), cost_c.cpu().numpy())


def _score_record(counts, totals, cost_c) -> dict:
    """The record ``score`` returns, from the host copies of counts int64 [5, 13] = (tp, fp, fn, r, k) per class, totals
    int64 [3] = (S, D, I) and cost_c float64 [13]."""
    def div(a, b):
        return float(a) / float(b) if b else math.nan

    TP, FP, FN, N, K = (int(v) for v in counts.sum(1))
    S, D, I = (int(v) for v in totals)
    per_class = {"TP": counts[0].tolist(), "FP": counts[1].tolist(), "FN": counts[2].tolist(), "N": counts[3].tolist(),
                 "F20": [div(2 * t, 2 * t + f + n) for t, f, n in zip(counts[0], counts[1], counts[2])],
                 "LE_CD": [div(c, kk) for c, kk in zip(cost_c, counts[4])],
                 "LR_CD": [div(kk, n) for kk, n in zip(counts[4], counts[3])]}
    return {"F20": div(2 * TP, 2 * TP + FP + FN), "ER20": div(S + D + I, N), "LE_CD": div(float(cost_c.sum()), K),
            "LR_CD": div(K, N), "TP": TP, "FP": FP, "FN": FN, "N": N, "S": S, "D": D, "I": I, "matched": K,
            "per_class": per_class}


def device_references(table: MetaFrameTable, metadata_rows, device):
    """``reference_table`` on ``device``: (offsets int32 [Q * 13 + 1], dirs int32 [R, 2])."""
    offsets, dirs = reference_table(table, metadata_rows)
    return torch.from_numpy(offsets).to(device), torch.from_numpy(dirs).to(device)


def refine_setting(refine) -> bool:
    """``refine`` as evaluate_logits takes it -> bool; None reads Config.SELD_REFINE."""
    from config import Config
    return bool(getattr(Config, "SELD_REFINE", False)) if refine is None else bool(refine)


def match_and_score(det_cell: torch.Tensor, det_count: torch.Tensor, table: MetaFrameTable, metadata_rows,
                    doa_threshold_deg: float, I: int = GRID_I, J: int = GRID_J, det_dir: torch.Tensor | None = None,
                    refine=None, refs=None) -> dict:
    """References (numpy CSR) -> seld_doa_match on the detections' device -> score().
    ``det_dir`` with ``refine`` (None reads Config.SELD_REFINE when ``det_dir`` is given): the detections' directions
    f32 [Q, 13, K, 2] are matched by seld_doa_match_dirs in place of the cell centres.
    ``refs``: what ``device_references`` returned for this timeline, for a caller that matches more than once."""
    if det_dir is None and refine:
        raise ValueError("match_and_score: refine needs det_dir (decode(..., refine=True))")
    refine = det_dir is not None and refine_setting(refine)
    offsets, dirs = device_references(table, metadata_rows, det_cell.device) if refs is None else refs
    if refine:
        stats, cost = doa_match_dirs(det_dir, det_count, offsets, dirs, doa_threshold_deg)
    else:
        stats, cost = doa_match(det_cell, det_count, offsets, dirs, doa_threshold_deg, I, J)
    return score(stats, cost)


# ------------------------------------------------------------------------------------------------------ threshold sweep

MAX_SWEEP = 64             # thresholds one seld_sweep_score launch takes (one lane each)
SWEEP_CHUNK = 64           # meta-frames per partial sum of seld_sweep_score
THRESHOLDS_VERSION = 1     # of the thresholds file


def _f32(value) -> float:
    """``value`` rounded once to fp32, as a Python float: the number the decode and the sweep kernel compare against."""
    return float(np.float32(value))


def parse_sweep(spec) -> tuple:
    """The thresholds of a sweep, ascending, each rounded once to fp32.  ``spec``: None, () or "" (off: returns ()), a
    sequence of numbers, or a string: "start:stop:step" (inclusive; "0.05:0.95:0.05" is 19 values) or a comma list
    ("0.1,0.25,0.5").  Raises ValueError for values outside (0, 1], duplicates (after the rounding) or more than 64."""
    if spec is None:
        return ()
    if isinstance(spec, str):
        text = spec.strip()
        if not text:
            return ()
        try:
            if ":" in text:
                parts = [float(v) for v in text.split(":")]
                if len(parts) != 3:
                    raise ValueError
                start, stop, step = parts
                if not (step > 0 and stop >= start):
                    raise ValueError
                n = int(math.floor((stop - start) / step + 1e-9)) + 1
                values = [round(start + i * step, 12) for i in range(n)]
            else:
                values = [float(v) for v in text.split(",") if v.strip()]
        except ValueError:
            raise ValueError(f"sweep: expected start:stop:step with step > 0 and stop >= start, or a comma list, got "
                             f"{spec!r}") from None
    else:
        values = [float(v) for v in spec]
    values = sorted(_f32(v) for v in values)
    if len(values) > MAX_SWEEP:
        raise ValueError(f"sweep: at most {MAX_SWEEP} thresholds, got {len(values)}")
    if any(not (0.0 < v <= 1.0) for v in values):
        raise ValueError(f"sweep: thresholds must lie in (0, 1], got {values}")
    if any(b <= a for a, b in zip(values, values[1:])):
        raise ValueError(f"sweep: duplicate thresholds in {values}")
    return tuple(values)


def class_threshold_vector(values) -> list:
    """13 detection thresholds, one per class, each rounded once to fp32; ValueError unless 13 numbers in (0, 1]."""
    try:
        out = [_f32(v) for v in values]
    except TypeError:
        raise ValueError("class_thresholds: expected 13 numbers or the path of a thresholds file") from None
    if len(out) != NUM_EVENT_CLASSES or any(not (0.0 < v <= 1.0) for v in out):
        raise ValueError(f"class_thresholds: expected {NUM_EVENT_CLASSES} numbers in (0, 1], got {out}")
    return out


def apply_thresholds(det_cell: torch.Tensor, det_score: torch.Tensor, det_count: torch.Tensor, class_thresholds,
                     det_dir: torch.Tensor | None = None):
    """The detections of a decode at a lower threshold cut to per-class thresholds: each (q, c) list keeps its LEADING
    detections with score >= class_thresholds[c] (fp32, the decode's comparison) -- the lists are sorted by score, so this
    is what the decode at that threshold keeps -- and is restored to the decode's conventions
    past the new count (cell -1, score 0, direction 0).  Returns new tensors (det_cell, det_score, det_count) and, given
    ``det_dir``, det_dir; framework ops where the tensors live."""
    thr = torch.tensor(class_threshold_vector(class_thresholds), dtype=torch.float32, device=det_score.device)
    rank = torch.arange(int(det_score.shape[-1]), device=det_score.device)
    ok = (rank < det_count[..., None]) & (det_score >= thr[None, :, None])
    keep = torch.cumprod(ok.to(torch.int32), dim=-1).bool()
    out = (torch.where(keep, det_cell, torch.full_like(det_cell, -1)),
           torch.where(keep, det_score, torch.zeros_like(det_score)), keep.sum(-1).to(det_count.dtype))
    if det_dir is not None:
        out += (torch.where(keep[..., None], det_dir, torch.zeros_like(det_dir)),)
    return out


def doa_match_prefix(det_cell: torch.Tensor, det_count: torch.Tensor, ref_offsets: torch.Tensor, ref_dirs: torch.Tensor,
                     doa_threshold_deg: float, I: int = GRID_I, J: int = GRID_J, det_dir: torch.Tensor | None = None):
    """seld_doa_match_prefix: (ptp int32 [Q, 13, K + 1], pcost f64 [Q, 13, K + 1]); entry p is the tp and cost of
    ``doa_match`` (``doa_match_dirs`` given ``det_dir`` f32 [Q, 13, K, 2]) with the entry's count replaced by p, entries
    past the count repeat the one at the count."""
    index, device, q, k, det_cell, det_dir, det_count, ref_offsets, dirs = _match_inputs(
        "doa_match_prefix", det_cell, det_dir, det_count, ref_offsets, ref_dirs)
    ptp = torch.empty((q, NUM_EVENT_CLASSES, k + 1), dtype=torch.int32, device=device)
    pcost = torch.empty((q, NUM_EVENT_CLASSES, k + 1), dtype=torch.float64, device=device)
    with _device_guard(index):
        check(load_library().seld_doa_match_prefix(_p(det_cell), _p(det_dir), _p(det_count), k, _p(ref_offsets), _p(dirs),
                                                   q, int(I), int(J), float(doa_threshold_deg) + DOA_MARGIN_DEG, _p(ptp),
                                                   _p(pcost), _stream_ptr(device)), "seld_doa_match_prefix")
    return ptp, pcost


def sweep_score(ptp: torch.Tensor, pcost: torch.Tensor, det_score: torch.Tensor, det_count: torch.Tensor,
                ref_offsets: torch.Tensor, thresholds, chunk: int = SWEEP_CHUNK):
    """seld_sweep_score: per threshold and per chunk of ``chunk`` consecutive meta-frames (counts int64 [T, n_chunks, 13,
    5] = (tp, fp, fn, r, k) per class, sdi int64 [T, n_chunks, 3], cost f64 [T, n_chunks, 13]).  ``thresholds`` go to the
    kernel as fp32 and are checked by the library (1..64 of them, strictly ascending, in (0, 1]: SeldNativeError)."""
    device = ptp.device
    if not ptp.is_cuda:
        raise SeldNativeError("sweep_score: the prefix tables must live on the GPU (no CPU fallback)")
    q, k = int(det_score.shape[0]), int(det_score.shape[-1])
    if tuple(ptp.shape) != (q, NUM_EVENT_CLASSES, k + 1) or tuple(pcost.shape) != tuple(ptp.shape) or \
            tuple(det_score.shape) != (q, NUM_EVENT_CLASSES, k) or tuple(det_count.shape) != (q, NUM_EVENT_CLASSES):
        raise ValueError("sweep_score: expected ptp / pcost [Q, 13, K + 1], det_score [Q, 13, K], det_count [Q, 13]")
    if ref_offsets.numel() != q * NUM_EVENT_CLASSES + 1:
        raise ValueError("sweep_score: ref_offsets must have Q * 13 + 1 entries")
    if int(chunk) < 1:
        raise ValueError("sweep_score: chunk must be >= 1")
    thr = np.ascontiguousarray(np.asarray(list(thresholds), dtype=np.float32).reshape(-1))
    index = ensure_init(device)
    t, n_chunks = len(thr), (q + int(chunk) - 1) // int(chunk)
    counts = torch.empty((t, n_chunks, NUM_EVENT_CLASSES, 5), dtype=torch.int64, device=device)
    sdi = torch.empty((t, n_chunks, 3), dtype=torch.int64, device=device)
    cost = torch.empty((t, n_chunks, NUM_EVENT_CLASSES), dtype=torch.float64, device=device)
    ptp, pcost = ptp.to(torch.int32).contiguous(), pcost.to(torch.float64).contiguous()
    det_score, det_count = det_score.to(torch.float32).contiguous(), det_count.to(torch.int32).contiguous()
    ref_offsets = ref_offsets.to(torch.int32).contiguous()
    with _device_guard(index):
        check(load_library().seld_sweep_score(_p(ptp), _p(pcost), _p(det_score), _p(det_count), k, _p(ref_offsets), q,
                                              thr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), t, int(chunk),
                                              _p(counts), _p(sdi), _p(cost), _stream_ptr(device)), "seld_sweep_score")
    return counts, sdi, cost


def _nan_last(value) -> float:
    return math.inf if value is None or math.isnan(value) else float(value)


def select_best(thresholds, f20, er20, per_class_f20, per_class_n) -> dict:
    """The operating points of a sweep: {"global": threshold or None, "per_class": [13 thresholds or None]}.  "global" is
    the threshold with the highest F20; ties go to the lower ER20 (nan last), then to the lower threshold; a nan F20
    never wins, None when every F20 is nan.  "per_class"[c] is chosen the same way on the class's own F20
    (per_class_f20[t][c]); a class without references (per_class_n[t][c] == 0) takes the global value."""
    def pick(scores):
        rows = [(-s, _nan_last(e), t) for s, e, t in zip(scores, er20, thresholds) if not math.isnan(s)]
        return min(rows)[2] if rows else None

    best = pick(f20)
    per_class = []
    for c in range(NUM_EVENT_CLASSES):
        own = pick([row[c] for row in per_class_f20]) if any(int(row[c]) for row in per_class_n) else None
        per_class.append(best if own is None else own)
    return {"global": best, "per_class": per_class}


def _sweep_result(thresholds, records) -> dict:
    """One ``score`` record per threshold -> the sweep's result: score's keys with lists over the thresholds, plus
    "thresholds", "precision", "recall" and "best" (``select_best``)."""
    def div(a, b):
        return float(a) / float(b) if b else math.nan

    out = {"thresholds": [float(t) for t in thresholds]}
    for key in records[0]:
        if key == "per_class":
            out[key] = {name: [rec[key][name] for rec in records] for name in records[0][key]}
        else:
            out[key] = [rec[key] for rec in records]
    out["precision"] = [div(rec["TP"], rec["TP"] + rec["FP"]) for rec in records]
    out["recall"] = [div(rec["TP"], rec["TP"] + rec["FN"]) for rec in records]
    out["best"] = select_best(out["thresholds"], out["F20"], out["ER20"], out["per_class"]["F20"], out["per_class"]["N"])
    return out


def sweep(det_cell: torch.Tensor, det_score: torch.Tensor, det_count: torch.Tensor, table: MetaFrameTable, metadata_rows,
          thresholds, doa_threshold_deg: float, I: int = GRID_I, J: int = GRID_J, det_dir: torch.Tensor | None = None,
          refs=None, chunk: int = SWEEP_CHUNK) -> dict:
    """Every threshold of ``thresholds`` (``parse_sweep``) scored from ONE decode at or below the lowest of them
    (DESIGN.md section 17): seld_doa_match_prefix, seld_sweep_score, one sum over the chunks.  Returns score's keys with
    lists over the thresholds -- row t is ``score`` of the detections ``apply_thresholds`` leaves at thresholds[t] (the
    costs to the last bits: they are summed in another shape) -- plus "thresholds", "precision", "recall" and "best".
    ``det_dir``: the detections' refined directions, matched in place of the cell centres.  ``refs``: as match_and_score."""
    thresholds = parse_sweep(thresholds)
    if not thresholds:
        raise ValueError("sweep: no thresholds")
    offsets, dirs = device_references(table, metadata_rows, det_count.device) if refs is None else refs
    ptp, pcost = doa_match_prefix(det_cell, det_count, offsets, dirs, doa_threshold_deg, I, J, det_dir=det_dir)
    counts, sdi, cost = sweep_score(ptp, pcost, det_score, det_count, offsets, thresholds, chunk)
    counts, sdi, cost = counts.sum(1).cpu().numpy(), sdi.sum(1).cpu().numpy(), cost.sum(1).cpu().numpy()
    return _sweep_result(thresholds, [_score_record(counts[t].T, sdi[t], cost[t]) for t in range(len(thresholds))])


_sweep = sweep             # (evaluate_logits has a parameter of that name)


def write_thresholds(path, swept: dict, max_peaks: int, doa_threshold_deg: float, tta_patterns=(), refine: bool = False,
                     tracking=None) -> Path:
    """The operating points of a sweep as a JSON file: version, global, per_class [13], the settings they were found
    under (max_peaks, doa_threshold_deg, tta_patterns, refine, tracking) and the swept grid with its F20 / ER20 (nan
    written as null).  ValueError when the sweep has no best threshold (every F20 nan)."""
    import json
    best = swept["best"]
    if best["global"] is None:
        raise ValueError("write_thresholds: every F20 of the sweep is nan (no references and no detections?)")

    def clean(values):
        return [None if math.isnan(v) else float(v) for v in values]

    tracking = {k: tracking[k] for k in ("gate_deg", "max_gap", "min_len")} if tracking else None
    doc = {"version": THRESHOLDS_VERSION, "global": float(best["global"]),
           "per_class": [float(v) for v in best["per_class"]], "max_peaks": int(max_peaks),
           "doa_threshold_deg": float(doa_threshold_deg), "tta_patterns": [int(p) for p in tta_patterns],
           "refine": bool(refine), "tracking": tracking,
           "grid": {"thresholds": [float(t) for t in swept["thresholds"]], "F20": clean(swept["F20"]),
                    "ER20": clean(swept["ER20"])}}
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(doc, indent=1) + "\n")
    return path


def load_thresholds(path, max_peaks=None, tta_patterns=None, refine=None) -> dict:
    """A thresholds file (``write_thresholds``) validated: version, "global" in (0, 1] and 13 "per_class" values in
    (0, 1], each returned rounded to fp32 (what they were when written).  ValueError otherwise.  Given the run's
    ``max_peaks`` / ``tta_patterns`` / ``refine``, warns (UserWarning) when the file was found under other settings: the
    best operating point moves with them."""
    import json
    import warnings
    path = Path(path)
    try:
        doc = json.loads(path.read_text())
    except (OSError, ValueError) as exc:
        raise ValueError(f"{path}: not a readable thresholds file ({exc})") from None
    if not isinstance(doc, dict) or doc.get("version") != THRESHOLDS_VERSION:
        raise ValueError(f"{path}: expected a thresholds file of version {THRESHOLDS_VERSION}")
    for key in ("global", "per_class", "max_peaks", "doa_threshold_deg", "tta_patterns", "refine"):
        if key not in doc:
            raise ValueError(f"{path}: missing \"{key}\"")
    glob = doc["global"]
    if isinstance(glob, bool) or not isinstance(glob, (int, float)) or not (0.0 < glob <= 1.0):
        raise ValueError(f"{path}: \"global\" must be a number in (0, 1]")
    per_class = doc["per_class"]
    if not isinstance(per_class, list) or len(per_class) != NUM_EVENT_CLASSES or \
            any(isinstance(v, bool) or not isinstance(v, (int, float)) or not (0.0 < v <= 1.0) for v in per_class):
        raise ValueError(f"{path}: \"per_class\" must be {NUM_EVENT_CLASSES} numbers in (0, 1]")
    doc = dict(doc, per_class=class_threshold_vector(per_class))
    doc["global"] = _f32(glob)
    run = {"max_peaks": None if max_peaks is None else int(max_peaks),
           "tta_patterns": None if tta_patterns is None else [int(p) for p in tta_patterns],
           "refine": None if refine is None else bool(refine)}
    for key, value in run.items():
        if value is not None and doc[key] != value:
            warnings.warn(f"{path}: thresholds were found with {key} = {doc[key]}, this run uses {value}; the best "
                          f"operating point moves with it", UserWarning, stacklevel=2)
    return doc


def sweep_setting(sweep) -> tuple:
    """``sweep`` as evaluate_logits takes it -> thresholds; None reads Config.SELD_SWEEP_THRESHOLDS."""
    from config import Config
    return parse_sweep(getattr(Config, "SELD_SWEEP_THRESHOLDS", ()) if sweep is None else sweep)


def class_thresholds_setting(class_thresholds, max_peaks=None, tta_patterns=None, refine=None):
    """``class_thresholds`` as evaluate_logits takes it -> 13 fp32 thresholds or None (off).  None reads
    Config.SELD_CLASS_THRESHOLDS; a str or Path is a thresholds file (``load_thresholds``, which warns when the file's
    settings are not the run's), else 13 numbers."""
    from config import Config
    if class_thresholds is None:
        class_thresholds = getattr(Config, "SELD_CLASS_THRESHOLDS", None)
    if class_thresholds is None:
        return None
    if isinstance(class_thresholds, (str, Path)):
        return load_thresholds(class_thresholds, max_peaks, tta_patterns, refine)["per_class"]
    return class_threshold_vector(class_thresholds)


# ------------------------------------------------------------------------------------------------------ segment metrics

BLOCK_FRAMES = 10          # meta-frames per block of the segment-based metrics: 1 s
SEG_STATS = ("Nref", "Npred", "TP", "FPs", "FP", "FN", "DE_TP", "DE_FN")      # seg_stats / the first eight of rec_counts
FIGURES = ("F", "ER", "LE", "LR", "SELD")


def block_table(table: MetaFrameTable) -> np.ndarray:
    """block_offsets int64 [S + 1] of a timeline: recording s has ceil(M_s / 10) blocks of 10 meta-frames (the last may be
    shorter), numbered block_offsets[s] .. block_offsets[s + 1] - 1."""
    frames = np.diff(table.seg_offsets)
    return np.concatenate([[0], np.cumsum((frames + BLOCK_FRAMES - 1) // BLOCK_FRAMES)]).astype(np.int64)


def doa_assign(det_cell: torch.Tensor, det_count: torch.Tensor, ref_offsets: torch.Tensor, ref_dirs: torch.Tensor,
               doa_threshold_deg: float, I: int = GRID_I, J: int = GRID_J, det_dir: torch.Tensor | None = None):
    """seld_doa_assign: pair_dist f64 [Q, 13, 8]; slot r of (q, c) is the distance of its reference r to the detection the
    minimum-cost assignment of ``doa_match`` (``doa_match_dirs`` given ``det_dir`` f32 [Q, 13, K, 2]) gives it, NaN when
    the reference is unassigned, absent or the entry refused."""
    index, device, q, k, det_cell, det_dir, det_count, ref_offsets, dirs = _match_inputs(
        "doa_assign", det_cell, det_dir, det_count, ref_offsets, ref_dirs)
    pair_dist = torch.empty((q, NUM_EVENT_CLASSES, MAX_REFS), dtype=torch.float64, device=device)
    with _device_guard(index):
        check(load_library().seld_doa_assign(_p(det_cell), _p(det_dir), _p(det_count), k, _p(ref_offsets), _p(dirs), q,
                                             int(I), int(J), float(doa_threshold_deg) + DOA_MARGIN_DEG, _p(pair_dist),
                                             _stream_ptr(device)), "seld_doa_assign")
    return pair_dist


def segment_score(pair_dist: torch.Tensor, det_count: torch.Tensor, max_peaks: int, ref_offsets: torch.Tensor,
                  table: MetaFrameTable, doa_threshold_deg: float):
    """seld_segment_score over the timeline of ``table``: (seg_stats int32 [NB, 13, 8] = SEG_STATS per (block, class),
    seg_de f64 [NB, 13], rec_counts int64 [S, 13, 11] = SEG_STATS and S_c, D_c, I_c per (recording, class), rec_sdi int64
    [S, 3], rec_de f64 [S, 13]).  ``max_peaks``: the K the counts are clamped to.  A slot counts as a true positive when its
    average distance over the block is <= doa_threshold_deg + DOA_MARGIN_DEG."""
    device = pair_dist.device
    if not pair_dist.is_cuda:
        raise SeldNativeError("segment_score: the assignment must live on the GPU (no CPU fallback)")
    q = len(table)
    if tuple(pair_dist.shape) != (q, NUM_EVENT_CLASSES, MAX_REFS) or tuple(det_count.shape) != (q, NUM_EVENT_CLASSES):
        raise ValueError(f"segment_score: expected pair_dist [{q}, 13, 8] and det_count [{q}, 13] for the timeline")
    if ref_offsets.numel() != q * NUM_EVENT_CLASSES + 1:
        raise ValueError("segment_score: ref_offsets must have Q * 13 + 1 entries")
    index = ensure_init(device)
    blocks = block_table(table)
    n_seg, n_blocks = len(blocks) - 1, int(blocks[-1])
    key = ("blocks", str(device))
    if key not in table._device:
        table._device[key] = torch.from_numpy(blocks).to(device)
    seg_offsets, block_offsets = table.device_segments(device)[0], table._device[key]
    seg_stats = torch.empty((n_blocks, NUM_EVENT_CLASSES, len(SEG_STATS)), dtype=torch.int32, device=device)
    seg_de = torch.empty((n_blocks, NUM_EVENT_CLASSES), dtype=torch.float64, device=device)
    rec_counts = torch.empty((n_seg, NUM_EVENT_CLASSES, len(SEG_STATS) + 3), dtype=torch.int64, device=device)
    rec_sdi = torch.empty((n_seg, 3), dtype=torch.int64, device=device)
    rec_de = torch.empty((n_seg, NUM_EVENT_CLASSES), dtype=torch.float64, device=device)
    pair_dist, det_count = pair_dist.to(torch.float64).contiguous(), det_count.to(torch.int32).contiguous()
    ref_offsets = ref_offsets.to(torch.int32).contiguous()
    with _device_guard(index):
        check(load_library().seld_segment_score(_p(pair_dist), _p(det_count), int(max_peaks), _p(ref_offsets),
                                                _p(seg_offsets), _p(block_offsets), n_seg,
                                                float(doa_threshold_deg) + DOA_MARGIN_DEG, _p(seg_stats), _p(seg_de),
                                                _p(rec_counts), _p(rec_sdi), _p(rec_de), _stream_ptr(device)),
              "seld_segment_score")
    return seg_stats, seg_de, rec_counts, rec_sdi, rec_de


def jackknife_score(rec_counts: torch.Tensor, rec_sdi: torch.Tensor, rec_de: torch.Tensor):
    """seld_jackknife_score: (out f64 [S + 1, 2, 5] = (micro, macro) x FIGURES, row j the metrics of every recording but
    j and row S those of all; out_class f64 [13, 5], the per-class figures of all recordings)."""
    device = rec_counts.device
    if not rec_counts.is_cuda:
        raise SeldNativeError("jackknife_score: the counts must live on the GPU (no CPU fallback)")
    n_seg = int(rec_counts.shape[0])
    if tuple(rec_counts.shape) != (n_seg, NUM_EVENT_CLASSES, len(SEG_STATS) + 3) or tuple(rec_sdi.shape) != (n_seg, 3) or \
            tuple(rec_de.shape) != (n_seg, NUM_EVENT_CLASSES):
        raise ValueError("jackknife_score: expected rec_counts [S, 13, 11], rec_sdi [S, 3], rec_de [S, 13]")
    index = ensure_init(device)
    out = torch.empty((n_seg + 1, 2, len(FIGURES)), dtype=torch.float64, device=device)
    out_class = torch.empty((NUM_EVENT_CLASSES, len(FIGURES)), dtype=torch.float64, device=device)
    rec_counts, rec_sdi = rec_counts.to(torch.int64).contiguous(), rec_sdi.to(torch.int64).contiguous()
    rec_de = rec_de.to(torch.float64).contiguous()
    with _device_guard(index):
        check(load_library().seld_jackknife_score(_p(rec_counts), _p(rec_sdi), _p(rec_de), n_seg, _p(out), _p(out_class),
                                                  _stream_ptr(device)), "seld_jackknife_score")
    return out, out_class


def _betacf(a: float, b: float, x: float) -> float:
    """The continued fraction of the regularised incomplete beta function (modified Lentz)."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 10000):
        m2 = 2 * m
        for num in (m * (b - m) * x / ((qam + m2) * (a + m2)), -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + num * d
            d = 1.0 / (d if abs(d) > tiny else tiny)
            c = 1.0 + num / c
            c = c if abs(c) > tiny else tiny
            h *= d * c
        if abs(d * c - 1.0) < 1e-16:
            break
    return h


def _betainc(a: float, b: float, x: float) -> float:
    """The regularised incomplete beta function I_x(a, b)."""
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _betacf(a, b, x) / a
    return 1.0 - front * _betacf(b, a, 1.0 - x) / b


@functools.lru_cache(maxsize=None)
def student_t_975(df) -> float:
    """The 0.975 quantile of Student's t with ``df`` >= 1 degrees of freedom, in plain Python: the distribution function
    through the incomplete beta function, inverted by bisection (about a millisecond; kept per ``df``)."""
    df = float(df)
    if not df >= 1.0:
        raise ValueError(f"student_t_975: df must be at least 1, got {df}")
    if df == 1.0:
        return math.tan(math.pi * 0.475)
    if df == 2.0:
        return 0.95 * math.sqrt(2.0 / (1.0 - 0.95 * 0.95))
    lo, hi = 1.9, 13.0                           # the quantile falls from 12.71 (df = 1) to 1.96 (df -> inf)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        upper_tail = 0.5 * _betainc(0.5 * df, 0.5, df / (df + mid * mid))
        lo, hi = (mid, hi) if upper_tail > 0.025 else (lo, mid)
    return 0.5 * (lo + hi)


def jackknife(values) -> dict:
    """The delete-one jackknife of one figure, float64.  ``values``: the n replicates theta_(i),
    then theta-hat of all recordings last (a row of ``jackknife_score``'s output).  nan replicates are dropped and n
    reduced with them.  Returns {estimate, bias, se, low, high, n}: bias = (n - 1)(mean - theta-hat), estimate =
    theta-hat - bias, se = sqrt((n - 1) / n * sum (theta_(i) - mean)^2), the interval estimate -+ t se with t the 0.975
    quantile of Student's t with n - 1 degrees of freedom.  Fewer than 2 usable replicates: estimate = theta-hat, the
    rest nan."""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    if values.size < 1:
        raise ValueError("jackknife: expected the replicates and the all-recordings figure")
    full, rep = float(values[-1]), values[:-1]
    rep = rep[~np.isnan(rep)]
    n = int(rep.size)
    if n < 2:
        return {"estimate": full, "bias": math.nan, "se": math.nan, "low": math.nan, "high": math.nan, "n": n}
    mean = float(rep.mean())
    bias = (n - 1) * (mean - full)
    se = math.sqrt((n - 1) / n * float(((rep - mean) ** 2).sum()))
    estimate, t = full - bias, student_t_975(n - 1)
    return {"estimate": estimate, "bias": bias, "se": se, "low": estimate - t * se, "high": estimate + t * se, "n": n}


_jackknife = jackknife     # (segment_metrics and evaluate_logits have a parameter of that name)


def segment_setting(segment, jackknife) -> tuple:
    """``segment`` / ``jackknife`` as evaluate_logits takes them -> (bool, bool); None reads Config.SELD_SEGMENT_METRICS /
    Config.SELD_JACKKNIFE.  ValueError for the jackknife without the segment metrics."""
    from config import Config
    segment = bool(getattr(Config, "SELD_SEGMENT_METRICS", False)) if segment is None else bool(segment)
    jackknife = bool(getattr(Config, "SELD_JACKKNIFE", False)) if jackknife is None else bool(jackknife)
    if jackknife and not segment:
        raise ValueError("jackknife needs the segment metrics (segment=True or Config.SELD_SEGMENT_METRICS)")
    return segment, jackknife


def segment_metrics(det_cell: torch.Tensor, det_count: torch.Tensor, table: MetaFrameTable, metadata_rows,
                    doa_threshold_deg: float, I: int = GRID_I, J: int = GRID_J, det_dir: torch.Tensor | None = None,
                    refs=None, jackknife: bool = False) -> dict:
    """The segment-based metrics of DESIGN.md section 18 for the detections of a timeline: seld_doa_assign,
    seld_segment_score, seld_jackknife_score, one copy of the small results to the host.  Returns "micro" and "macro"
    ({F, ER, LE, LR, SELD}), "per_class" (the figures and the counts as lists over the classes), "counts" (SEG_STATS and the
    micro S, D, I over all recordings), "classes" (those with references, which the macro average runs over), "blocks",
    "recordings" and "block_seconds"; with ``jackknife`` also "ci": per average and figure ``jackknife``'s record over the
    recordings.  ``det_dir``: the detections' refined directions, matched in place of the cell centres.  ``refs``: as
    match_and_score."""
    n_seg = len(table.seg_offsets) - 1
    if n_seg < 1:
        raise ValueError("segment_metrics: the timeline has no recordings")
    offsets, dirs = device_references(table, metadata_rows, det_count.device) if refs is None else refs
    k = int(det_dir.shape[2] if det_dir is not None else det_cell.shape[-1])
    pair_dist = doa_assign(det_cell, det_count, offsets, dirs, doa_threshold_deg, I, J, det_dir=det_dir)
    seg_stats, _, rec_counts, rec_sdi, rec_de = segment_score(pair_dist, det_count, k, offsets, table, doa_threshold_deg)
    out, out_class = jackknife_score(rec_counts, rec_sdi, rec_de)
    out, out_class = out.cpu().numpy(), out_class.cpu().numpy()
    counts, sdi = rec_counts.sum(0).cpu().numpy(), rec_sdi.sum(0).cpu().numpy()        # [13, 11], [3]
    names = SEG_STATS + ("S", "D", "I")
    per_class = {name: [float(v) for v in out_class[:, i]] for i, name in enumerate(FIGURES)}
    per_class.update({name: [int(v) for v in counts[:, i]] for i, name in enumerate(names)})
    totals = {name: int(counts[:, i].sum()) for i, name in enumerate(SEG_STATS)}
    totals.update(S=int(sdi[0]), D=int(sdi[1]), I=int(sdi[2]))
    result = {"micro": {name: float(out[-1, 0, i]) for i, name in enumerate(FIGURES)},
              "macro": {name: float(out[-1, 1, i]) for i, name in enumerate(FIGURES)},
              "per_class": per_class, "counts": totals, "classes": [c for c in range(NUM_EVENT_CLASSES) if counts[c, 0] > 0],
              "blocks": int(seg_stats.shape[0]), "recordings": n_seg, "block_seconds": BLOCK_FRAMES * 0.1}
    if jackknife:
        result["ci"] = {avg: {name: _jackknife(out[:, a, i]) for i, name in enumerate(FIGURES)}
                        for a, avg in enumerate(("micro", "macro"))}
    return result


# ------------------------------------------------------------------------------------------------------ events

def events_for_segment(det_cell, det_count, table: MetaFrameTable, segment: int, I: int = GRID_I, J: int = GRID_J,
                       ids=None, dirs=None):
    """Event rows of one segment: int32 [R, 5] = (meta_frame, class, rank, azimuth, elevation) in (m, c, rank) order,
    the DOA being the detection's cell centre (integer degrees on the 10-degree grid).
    ``ids``: the track ids that go with ``det_cell`` (``track``'s trk_id next to trk_cell / trk_count); the third column
    is then the track id, rows in (m, c, id) order -- the order ``track`` writes them in.
    ``dirs``: the refined directions that go with ``det_cell`` (f32 [Q, 13, K, 2] degrees); the DOA
    is then their nearest integer degree, an azimuth that rounds to 180 written as -180."""
    lo, hi = int(table.seg_offsets[segment]), int(table.seg_offsets[segment + 1])
    cells = det_cell[lo:hi].cpu().numpy() if torch.is_tensor(det_cell) else np.asarray(det_cell)[lo:hi]
    count = det_count[lo:hi].cpu().numpy() if torch.is_tensor(det_count) else np.asarray(det_count)[lo:hi]
    m, c, rank = np.meshgrid(np.arange(hi - lo), np.arange(NUM_EVENT_CLASSES), np.arange(cells.shape[-1]), indexing="ij")
    sel = rank < count[..., None]
    cell = cells[sel].astype(np.int64)
    az = np.rint(-180.0 + (cell % J + 0.5) * (360.0 / J))
    el = np.rint(-90.0 + (cell // J + 0.5) * (180.0 / I))
    if dirs is not None:
        d = dirs[lo:hi].cpu().numpy() if torch.is_tensor(dirs) else np.asarray(dirs)[lo:hi]
        az, el = np.rint(d[..., 0][sel].astype(np.float64)), np.rint(d[..., 1][sel].astype(np.float64))
        az = np.where(az >= 180.0, az - 360.0, az)
    if ids is not None:
        rank = ids[lo:hi].cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)[lo:hi]
    return np.stack([m[sel], c[sel], rank[sel], az, el], axis=1).astype(np.int32).reshape(-1, 5)


def tracks_for_segment(tracks, chain_tracks, chain_offsets, segment: int):
    """Rows of one segment's kept tracks: int32 [R, 5] = (class, track, onset_m, offset_m, detected_frames) in (class,
    track) order, from the host copies of ``track``'s tracks / chain_tracks / chain_offsets; onset and offset are meta-frame
    indices, both inclusive.  Five integer columns, so write_events_csv writes them."""
    rows = []
    for c in range(NUM_EVENT_CLASSES):
        x = segment * NUM_EVENT_CLASSES + c
        part = np.asarray(tracks)[int(chain_offsets[x]):int(chain_offsets[x]) + int(chain_tracks[x])]
        for tid in np.nonzero(part[:, 3])[0]:
            rows.append([c, int(tid), int(part[tid, 0]), int(part[tid, 1]), int(part[tid, 2])])
    return np.array(rows, dtype=np.int32).reshape(-1, 5)


def write_events_csv(path, rows) -> Path:
    """One ``m,c,rank,az,el`` line per event, the reference's 5-column metadata format (dataset._read_metadata_rows reads
    it back unchanged)."""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    with open(path, "w", newline="") as fh:
        fh.writelines(",".join(str(int(v)) for v in row) + "\n" for row in rows)
    return path


def segment_names(dataset):
    """The audio stems of the dataset's files, or segment0000, segment0001, ... for an in-memory timeline."""
    files = list(getattr(dataset, "audio_files", None) or [])
    n = len(dataset.segments)
    return [Path(f).stem for f in files] if len(files) == n else [f"segment{s:04d}" for s in range(n)]


# ------------------------------------------------------------------------------------------------------ entry point

# the detections of a timeline as evaluate_logits hands them on; dir (the refined directions) is None without refine
Detections = namedtuple("Detections", "cell score count dir", defaults=(None,))


def evaluate_logits(batches, dataset, threshold=None, max_peaks=None, doa_threshold_deg=None, events_dir=None,
                    names=None, patterns=None, track=None, refine=None, sweep=None, class_thresholds=None,
                    thresholds_out=None, segment=None, jackknife=None) -> dict:
    """Decode + score for any iterator of logit batches [B, 250, 648, 14] that covers ``dataset``'s windows in order.
    ``dataset``: an SELDDataset (``segments``, ``metadata_rows``, ``total_frames``, ``I``, ``J``, ``device``).  Defaults
    come from Config (SELD_THRESHOLD, SELD_MAX_PEAKS, SELD_DOA_THRESHOLD_DEG).  Returns F20, ER20, LE_CD, LR_CD, TP, FP,
    FN, N, per_class (plus S, D, I, matched and the settings); with ``events_dir`` one CSV per segment, named after
    ``names`` or the audio stems, listed under "event_files".
    ``patterns``: test-time augmentation (``decode``): the batches are [P, B, 250, 648, 14]; the result's "tta_patterns"
    lists them ([] when off).
    ``track``: track linking of the decoded detections.  None reads Config.SELD_TRACK; True or a
    dict with any of gate_deg, max_gap, min_len (defaults: Config.SELD_TRACK_*) switches it on: the whole timeline is
    decoded, linked into tracks (``track``) and the surviving emissions are what is scored and written.  The result's
    "tracking" is then {gate_deg, max_gap, min_len, tracks, tracks_kept, filled, removed}, else None; the CSV rows are
    ``m,c,track_id,az,el`` and ``<name>.tracks.csv`` (class, track, onset_m, offset_m, detected_frames of the kept
    tracks) is written next to each, listed under "track_files".
    ``refine``: sub-cell DOA refinement.  None reads Config.SELD_REFINE; True decodes with
    ``grid_decode_refine``, scores the detections' refined directions (seld_doa_match_dirs) and writes their nearest
    integer degrees to the CSVs in place of the cell centres.  With ``track`` the linking itself stays on cells; a
    surviving emission takes the refined direction of the detection it is, a filled one its cell centre
    (``track_dirs``).  The result's "refine" says which.
    ``sweep``: a threshold sweep.  None reads Config.SELD_SWEEP_THRESHOLDS (() = off); else a
    sequence of thresholds or a spelling ``parse_sweep`` takes ("0.05:0.95:0.05").  The timeline is decoded ONCE, at the
    lowest of the swept thresholds and ``threshold``; the main result is still the one at ``threshold``
    (``apply_thresholds``) and gains "sweep": score's keys with lists over the thresholds, "thresholds", "precision",
    "recall" and "best" (``sweep``) -- row t is what evaluate_logits(threshold=t) returns.  With ``track`` the link
    depends on the threshold, so each row is cut, linked and matched in turn.
    ``class_thresholds``: one detection threshold per class in place of ``threshold`` (giving both raises ValueError).
    None reads Config.SELD_CLASS_THRESHOLDS; else 13 numbers or the path of a thresholds file.  The timeline is decoded at
    their minimum and cut per class before tracking, matching and the CSVs; the result carries "class_thresholds".
    ``thresholds_out``: with a sweep, write its best global / per-class thresholds, the settings and the swept grid to
    this file (``write_thresholds``; None reads Config.SELD_THRESHOLDS_OUT), listed under "thresholds_file".
    ``segment``: the segment-based, class-macro metrics of DESIGN.md section 18 (one decision per class and 1 s block,
    macro-averaged over the classes, one SELD score).  None reads Config.SELD_SEGMENT_METRICS; True adds "segment"
    (``segment_metrics``) for the detections the main result scores: after the class thresholds and tracking, on the
    refined directions with ``refine``.  The frame-wise keys are computed as ever; sweep rows do not gain it.
    ``jackknife``: with ``segment``, 95 % confidence intervals from the delete-one jackknife over the recordings, under
    "segment"["ci"] (None reads Config.SELD_JACKKNIFE; without ``segment`` ValueError)."""
    from config import Config
    segment, jackknife = segment_setting(segment, jackknife)
    tracking = track_settings(track)
    refine = refine_setting(refine)
    patterns = tuple(int(p) for p in patterns) if patterns is not None else ()
    max_peaks = Config.SELD_MAX_PEAKS if max_peaks is None else max_peaks
    swept = sweep_setting(sweep)
    if thresholds_out is not None and not swept:
        raise ValueError("thresholds_out needs a sweep (sweep=... or Config.SELD_SWEEP_THRESHOLDS)")
    if thresholds_out is None and swept:
        thresholds_out = getattr(Config, "SELD_THRESHOLDS_OUT", None)
    if class_thresholds is not None and threshold is not None:
        raise ValueError("give either threshold or class_thresholds, not both")
    # (an explicit threshold wins over Config.SELD_CLASS_THRESHOLDS)
    per_class = class_thresholds_setting(class_thresholds, max_peaks, patterns, refine) if threshold is None else None
    threshold = Config.SELD_THRESHOLD if threshold is None else threshold
    # the cut thresholds, fp32 as the decode compares them; None: the decode itself runs at ``threshold``, as ever
    cut = per_class if per_class is not None else [_f32(threshold)] * NUM_EVENT_CLASSES if swept else None
    decode_threshold = threshold if cut is None else min(list(swept) + cut)
    doa_threshold_deg = Config.SELD_DOA_THRESHOLD_DEG if doa_threshold_deg is None else doa_threshold_deg
    if (dataset.I, dataset.J) != (GRID_I, GRID_J):
        raise NotImplementedError(f"the decode kernel is built for the {GRID_I} x {GRID_J} grid, got "
                                  f"{dataset.I} x {dataset.J}")
    table = meta_frame_table(dataset.segments, dataset.total_frames)
    decoded = decode(batches, table, decode_threshold, max_peaks, device=dataset.device, patterns=patterns, refine=refine)
    low = Detections(decoded[0], decoded[1], decoded[2], decoded[4] if refine else None)    # at decode_threshold
    settings = tracking
    refs = device_references(table, dataset.metadata_rows, low.cell.device) if swept or segment else None

    def cut_to(thresholds):
        return Detections(*apply_thresholds(low.cell, low.score, low.count, thresholds, low.dir))

    def link_and_score(dets):
        """Detections -> (record, cell, ids, count, dir, linked, tracking)."""
        cell, count, dirs = dets.cell, dets.count, dets.dir
        ids = linked = None
        summary = settings
        if settings is not None:
            linked = _track_link(cell, count, table, settings["gate_deg"], settings["max_gap"], settings["min_len"],
                                 dataset.I, dataset.J)
            if refine:
                dirs = track_dirs(linked[0], linked[2], cell, count, dirs, dataset.I, dataset.J)
            cell, ids, count = linked[:3]
            summary = {**settings, **track_summary(linked[2], linked[3], linked[4])}
        record = match_and_score(cell, count, table, dataset.metadata_rows, doa_threshold_deg, dataset.I, dataset.J,
                                 det_dir=dirs, refine=refine, refs=refs)
        return record, cell, ids, count, dirs, linked, summary

    result, det_cell, ids, det_count, det_dir, linked, tracking = link_and_score(low if cut is None else cut_to(cut))
    result.update(threshold=float(threshold), max_peaks=int(max_peaks), doa_threshold_deg=float(doa_threshold_deg),
                  tta_patterns=list(patterns), tracking=tracking, refine=refine)
    if per_class is not None:
        result["class_thresholds"] = list(per_class)
    if segment:
        result["segment"] = segment_metrics(det_cell, det_count, table, dataset.metadata_rows, doa_threshold_deg,
                                            dataset.I, dataset.J, det_dir=det_dir, refs=refs, jackknife=jackknife)
    if swept:
        if settings is None:
            result["sweep"] = _sweep(low.cell, low.score, low.count, table, dataset.metadata_rows, swept,
                                     doa_threshold_deg, dataset.I, dataset.J, det_dir=low.dir, refs=refs)
        else:
            rows = [link_and_score(cut_to([t] * NUM_EVENT_CLASSES))[0] for t in swept]
            result["sweep"] = _sweep_result(swept, rows)
        if thresholds_out is not None:
            result["thresholds_file"] = str(write_thresholds(thresholds_out, result["sweep"], max_peaks, doa_threshold_deg,
                                                             patterns, refine, settings))
    if events_dir is not None:
        names = segment_names(dataset) if names is None else list(names)
        cells, counts = det_cell.cpu().numpy(), det_count.cpu().numpy()
        ids = ids.cpu().numpy() if ids is not None else None
        dirs = det_dir.cpu().numpy() if det_dir is not None else None
        result["event_files"] = [str(write_events_csv(Path(events_dir) / f"{name}.csv",
                                                      events_for_segment(cells, counts, table, s, dataset.I, dataset.J,
                                                                         ids=ids, dirs=dirs)))
                                 for s, name in enumerate(names)]
        if linked is not None:
            rows, born, offsets = (t.cpu().numpy() for t in linked[3:6])
            result["track_files"] = [str(write_events_csv(Path(events_dir) / f"{name}.tracks.csv",
                                                          tracks_for_segment(rows, born, offsets, s)))
                                     for s, name in enumerate(names)]
    return result
