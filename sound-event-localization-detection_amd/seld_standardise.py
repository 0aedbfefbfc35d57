"""Per-bin feature standardisation: the host side of Config.STANDARDISE_FEATURES.

The moments of the training timeline come from the device (``seld_native.feature_moments``, csrc/standardise.hip: sum x and
sum x^2 per (channel, bin) column in a fixed fp64 order); everything here is float64 (numpy) on the host and touches no GPU:

  ``finalise(moments, frames)``   moments -> statistics: mean, std and the fp32 tables the affine gathers read,
                                  out = fmaf(x, scale, shift) with scale = 1 / std, shift = -mean / std
  ``to_payload`` / ``from_payload``   the statistics as they travel in a checkpoint (key ``feature_statistics``): CPU float64
                                  tensors and plain values, never the live device tensors

Statistics are a dict: ``mean`` / ``std`` float64 [C, 64], ``frames`` int, ``scale`` / ``shift`` float32 [C, 64], all on
the CPU.  ``scale`` and ``shift`` are a pure function of (mean, std) -- ``affine_tables`` -- so a checkpoint that stores mean
and std reproduces them bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch

N_BINS = 64
FLAT_STD = 1e-6            # a bin whose standard deviation is below this is only centred (scale 1): dividing would blow up noise
PAYLOAD_KEYS = ("mean", "std", "frames", "feature_set", "channels")


def affine_tables(mean: torch.Tensor, std: torch.Tensor):
    """(scale, shift) float32 [C, 64] from float64 mean and std: 1 / std and -mean / std, each rounded to fp32 once; a flat
    bin (std < FLAT_STD) gets scale 1 and shift -mean."""
    mean, std = _table(mean, "mean"), _table(std, "std")
    if mean.shape != std.shape:
        raise ValueError(f"feature statistics: mean {tuple(mean.shape)} and std {tuple(std.shape)} differ in shape")
    if bool((std < 0).any()):
        raise ValueError("feature statistics: negative standard deviation")
    # numpy float64: IEEE division and rounding whatever the host's vector math library does (every rank of a data-parallel
    # run builds these tables itself and they must agree bit for bit)
    mean, std = mean.numpy(), std.numpy()
    flat = std < FLAT_STD
    safe = np.where(flat, 1.0, std)
    scale = np.where(flat, 1.0, 1.0 / safe).astype(np.float32)
    shift = np.where(flat, -mean, -mean / safe).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(scale)), torch.from_numpy(np.ascontiguousarray(shift))


def _table(value, what: str) -> torch.Tensor:
    t = torch.as_tensor(value).detach().to(device="cpu", dtype=torch.float64)
    if t.dim() != 2 or t.shape[1] != N_BINS or t.shape[0] < 1:
        raise ValueError(f"feature statistics: {what} must be [channels, {N_BINS}], got {tuple(t.shape)}")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"feature statistics: non-finite {what}")
    return t.contiguous()


def finalise(moments, frames: int) -> dict:
    """Moments float64 [2, C, 64] (sum x, sum x^2 over ``frames`` frames) -> statistics.  mean = S1 / T,
    var = max(S2 / T - mean^2, 0) (round-off can take the difference of a nearly flat bin below zero), std = sqrt(var).
    Non-finite moments raise: a NaN or inf in the timeline would otherwise standardise every batch to NaN."""
    frames = int(frames)
    if frames < 1:
        raise ValueError(f"feature statistics: frames must be positive, got {frames}")
    m = torch.as_tensor(moments).detach().to(device="cpu", dtype=torch.float64)
    if m.dim() != 3 or m.shape[0] != 2 or m.shape[2] != N_BINS or m.shape[1] < 1:
        raise ValueError(f"feature statistics: moments must be [2, channels, {N_BINS}], got {tuple(m.shape)}")
    if not bool(torch.isfinite(m).all()):
        raise ValueError("feature statistics: non-finite moments (the timeline holds a NaN or an infinity)")
    m = m.numpy()                  # numpy float64: a correctly rounded square root on every host (see affine_tables)
    mean = m[0] / frames
    var = np.maximum(m[1] / frames - mean * mean, 0.0)
    return statistics(torch.from_numpy(mean), torch.from_numpy(np.sqrt(var)), frames)


def statistics(mean, std, frames: int) -> dict:
    mean, std = _table(mean, "mean"), _table(std, "std")
    scale, shift = affine_tables(mean, std)
    return {"mean": mean, "std": std, "frames": int(frames), "scale": scale, "shift": shift}


def to_payload(stats: dict, feature_set: str, channels: int | None = None) -> dict:
    """What a checkpoint stores under ``feature_statistics``."""
    mean, std = _table(stats["mean"], "mean"), _table(stats["std"], "std")
    channels = int(mean.shape[0]) if channels is None else int(channels)
    if channels != int(mean.shape[0]):
        raise ValueError(f"feature statistics hold {int(mean.shape[0])} channels, not {channels}")
    return {"mean": mean.clone(), "std": std.clone(), "frames": int(stats["frames"]), "feature_set": str(feature_set),
            "channels": channels}


def from_payload(payload: dict, channels: int | None = None, feature_set: str | None = None) -> dict:
    """Statistics from a checkpoint's ``feature_statistics``; ``channels`` / ``feature_set``: what the caller's features are
    -- a mismatch raises (statistics of another feature set would silently de-normalise the input)."""
    missing = [k for k in PAYLOAD_KEYS if k not in payload]
    if missing:
        raise KeyError(f"feature_statistics payload lacks {', '.join(missing)}")
    stats = statistics(payload["mean"], payload["std"], payload["frames"])
    have = int(stats["mean"].shape[0])
    if int(payload["channels"]) != have:
        raise ValueError(f"feature_statistics payload says {payload['channels']} channels but holds {have}")
    if channels is not None and int(channels) != have:
        raise ValueError(f"feature statistics are for {have} feature channels ({payload['feature_set']!r}), the features "
                         f"have {int(channels)}")
    if feature_set is not None and str(feature_set) != str(payload["feature_set"]):
        raise ValueError(f"feature statistics are for FEATURE_SET {payload['feature_set']!r}, not {feature_set!r}")
    return stats


def checkpoint_statistics(checkpoint: dict, config, channels: int | None = None):
    """What evaluation applies: the checkpoint decides.  Its ``feature_statistics`` when it holds them (whatever the
    switch says: the weights were trained on standardised input); None when it holds none and Config.STANDARDISE_FEATURES is
    off; an error when the switch is on and the checkpoint has none -- never a silent evaluation on raw features."""
    payload = checkpoint.get("feature_statistics") if hasattr(checkpoint, "get") else None
    if payload is None:
        if bool(getattr(config, "STANDARDISE_FEATURES", False)):
            raise KeyError("STANDARDISE_FEATURES is set but the checkpoint holds no 'feature_statistics' (train with the "
                           "switch on)")
        return None
    return from_payload(payload, channels=channels)
