"""Dataset assembly for SELD training on MI355X (drop-in for the reference's ``dataset.py``).

Same public surface -- ``load_audio``, ``audio_to_mel_spectrogram``, ``metadata_to_labels``,
``load_files``, ``SELDDataset`` (``.I .J .total_cells``, ``len``, ``[i] -> (spec [250,C,64] f32,
labels [250,648,14] f32)``) -- so the reference's ``main.py`` runs unchanged, but the work is done
by the HIP kernels behind ``seld_native`` instead of torchaudio / pandas / Python loops:

  reference (dataset.py)                         here
  -------------------------------------------    -------------------------------------------------
  :18-25   torchaudio.load                       stdlib ``wave`` PCM reader (int16 kept as int16)
  :27-58   MelSpectrogram + AmplitudeToDB        seld_logmel_{f32,i16}: one fused kernel, written
                                                 time-major so a window is a contiguous slice
  :60-119  iterrows + T x 648 Python loops       seld_labels_rasterise -> uint16 class mask / cell
  :212-265 torch.cat of per-file tensors         one device timeline [sum T, C, 64] + [sum T, 648]
  :267-317 list of 250-frame dict views          window start table; seld_window_gather per batch

The dense [250,648,14] float labels the reference keeps in RAM (36 KB per frame) are only
materialised when an item is requested through ``__getitem__`` (stock DataLoader path); the
trainer's device feed uses the compact mask directly (``device_batch``).
"""
import csv
import logging
import wave
from glob import glob
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import Dataset

import seld_augment
import seld_native
import seld_standardise
from config import Config
from utils import polar_to_grid  # noqa: F401  (re-exported like the reference module)

logger = logging.getLogger("SMR_SELD")
config = Config()

FRAME_MS = 20
META_FRAME_MS = 100


# ------------------------------------------------------------------------------------ audio I/O

def _read_wav(audio_path):
    """PCM WAV -> (int array [C, L], sample_rate, bits).  16-bit stays int16 (fast path)."""
    with wave.open(str(audio_path), "rb") as wf:
        channels, width, rate, frames = wf.getnchannels(), wf.getsampwidth(), wf.getframerate(), wf.getnframes()
        raw = wf.readframes(frames)
    if width == 2:
        data = np.frombuffer(raw, dtype="<i2")
    elif width == 4:
        data = np.frombuffer(raw, dtype="<i4")
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        data = (b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16))
        data = np.where(data >= 1 << 23, data - (1 << 24), data)
    elif width == 1:
        data = np.frombuffer(raw, dtype=np.uint8).astype(np.int16) - 128
    else:
        raise ValueError(f"unsupported WAV sample width {width} in {audio_path}")
    return np.ascontiguousarray(data.reshape(-1, channels).T), rate, 8 * width


def load_audio(audio_path):
    """(waveform float32 [C, L] in [-1, 1), sample_rate) -- what ``torchaudio.load`` returns for a
    PCM file (dataset.py:18-25).  Warns when the file does not have 4 channels."""
    data, rate, bits = _read_wav(audio_path)
    waveform = torch.from_numpy(data.astype(np.float32) / float(1 << (bits - 1)))
    if waveform.shape[0] != 4:
        logger.warning(f"Expected 4 channels but got {waveform.shape[0]} channels in {audio_path}")
    return waveform, rate


def _nipd_settings():
    """(NIPD_MIN_HZ, NIPD_MAX_HZ, SOUND_SPEED) of FEATURE_SET 'logmel_nipd' as this module's config holds them."""
    return config.NIPD_MIN_HZ, config.NIPD_MAX_HZ, config.SOUND_SPEED


def _compute_device():
    if not torch.cuda.is_available():
        raise seld_native.SeldNativeError(
            "the SELD feature / label kernels need a ROCm GPU: there is no CPU fallback in the product path")
    return torch.device("cuda", torch.cuda.current_device())


def audio_to_mel_spectrogram(waveform, sample_rate, n_fft=None, hop_length=None, n_mels=None):
    """[C, L] waveform -> log-mel dB [C, n_mels, 1 + L // hop] (dataset.py:27-58), computed by the fused
    gfx950 kernel.  The kernel is specialised for the reference's configuration (24 kHz, n_fft 960,
    hop 480, 64 mels: config.py:85-88); anything else raises.  The result lives where the input lives."""
    n_fft = config.SPECTROGRAM_N_FFT if n_fft is None else n_fft
    hop_length = config.SPECTROGRAM_HOP_LENGTH if hop_length is None else hop_length
    n_mels = config.N_MELS if n_mels is None else n_mels
    convert = int(sample_rate) != 24000 and bool(getattr(config, "RESAMPLE_INPUT", False))
    if (24000 if convert else int(sample_rate), int(n_fft), int(hop_length), int(n_mels)) != (24000, 960, 480, 64):
        raise NotImplementedError(
            "the HIP log-mel kernel is built for sr=24000, n_fft=960, hop=480, n_mels=64 (config.py:85-88); "
            f"got sr={sample_rate}, n_fft={n_fft}, hop={hop_length}, n_mels={n_mels}")
    on_host = not waveform.is_cuda
    x = waveform.to(_compute_device()) if on_host else waveform
    if x.dtype not in (torch.float32, torch.int16):
        x = x.to(torch.float32)
    if convert:                                   # Config.RESAMPLE_INPUT: to 24 kHz on the device first
        x = seld_native.resample(x.contiguous(), int(sample_rate), 24000)
    out = seld_native.logmel(x, layout="cft")
    return out.cpu() if on_host else out


# ------------------------------------------------------------------------------------ labels

def _read_metadata_rows(metadata_path):
    """``pd.read_csv(path, header=None)`` + the int() casts of dataset.py:93-97 -> int64 [R, 5]."""
    rows = []
    with open(metadata_path, "r", newline="") as fh:
        for rec in csv.reader(fh):
            if rec:
                rows.append([int(float(v)) for v in rec[:5]])
    return np.asarray(rows, dtype=np.int64).reshape(-1, 5)


def label_frame_count(audio_duration):
    """dataset.py:73, same float64 operation order (NOT an integer division)."""
    return int((audio_duration * 1000) / FRAME_MS)


def _grid_dims(I, J, cell_size_deg):
    if (I is None or J is None) and cell_size_deg is not None:
        return int(180 // cell_size_deg), int(360 // cell_size_deg)
    if I is None or J is None:
        raise ValueError("Either provide (I, J) or cell_size_deg for grid dimensions")
    return I, J


def metadata_to_mask(metadata_path, audio_duration, I=None, J=None, cell_size_deg=None, device=None):
    """Compact form of ``metadata_to_labels``: uint16 [T, I*J] on the GPU, bit c = class c active."""
    cell_size_deg = config.GRID_CELL_DEGREES if cell_size_deg is None else cell_size_deg
    I, J = _grid_dims(I, J, cell_size_deg)
    rows = _read_metadata_rows(metadata_path) if not isinstance(metadata_path, np.ndarray) else metadata_path
    total_frames = label_frame_count(audio_duration)
    device = _compute_device() if device is None else device
    return seld_native.rasterise_labels(torch.from_numpy(np.ascontiguousarray(rows)), total_frames, I, J,
                                        device=device), I, J


def metadata_to_labels(metadata_path, audio_duration, sample_rate=24000, I=None, J=None,
                       cell_size_deg=None, num_classes=14):
    """CSV metadata -> (labels float32 [T, I*J, num_classes], I, J) as dataset.py:60-119 builds it,
    rasterised on the GPU (integer path, bit-exact) and returned on the host like the reference."""
    mask, I, J = metadata_to_mask(metadata_path, audio_duration, I, J, cell_size_deg)
    return seld_native.expand_labels(mask, num_classes).cpu(), I, J


def augment_with_gaussian_mask(metadata_path, audio_duration, I=None, J=None, cell_size_deg=None,
                               sigma_azimuth=5.0, sigma_elevation=5.0, device=None, rng=None):
    """Compact form of ``augment_with_gaussian_noise``: uint16 [T, I*J] on the GPU.  The per-source normal
    draws (smrl_seld_gaussian.py:426-437) come from ``rng`` (default ``numpy.random`` like the reference)."""
    cell_size_deg = config.GRID_CELL_DEGREES if cell_size_deg is None else cell_size_deg
    I, J = _grid_dims(I, J, cell_size_deg)
    rows = _read_metadata_rows(metadata_path) if not isinstance(metadata_path, np.ndarray) else metadata_path
    total_frames = label_frame_count(audio_duration)
    device = _compute_device() if device is None else device
    centres = seld_native.gaussian_source_noise(rows, sigma_azimuth, sigma_elevation, rng=rng)
    return seld_native.rasterise_labels_gaussian(torch.from_numpy(np.ascontiguousarray(rows)), centres, total_frames,
                                                 I, J, sigma_azimuth, sigma_elevation, device=device), I, J


def augment_with_gaussian_noise(metadata_path, audio_duration, sample_rate=24000, I=None, J=None,
                                cell_size_deg=None, num_classes=14, sigma_azimuth=5.0, sigma_elevation=5.0, rng=None):
    """smrl_seld_gaussian.py:397-534 with the same signature and return value: every source paints its class
    into all grid cells whose centre lies in the +-2 sigma box around its (noise-shifted) direction."""
    mask, I, J = augment_with_gaussian_mask(metadata_path, audio_duration, I, J, cell_size_deg, sigma_azimuth,
                                            sigma_elevation, rng=rng)
    return seld_native.expand_labels(mask, num_classes).cpu(), I, J


# ------------------------------------------------------------------------------------ file lists

def load_files():
    """(train_audio, train_meta, test_audio, test_meta) lists (dataset.py:121-165)."""
    if not config.USE_FULL_DATASET:
        return ([str(config.TRAIN_AUDIO_PATH)], [str(config.TRAIN_META_PATH)],
                [str(config.TEST_AUDIO_PATH)], [str(config.TEST_META_PATH)])

    def pair(audio_dir, meta_dir):
        audio = sorted(glob(str(audio_dir / "*.wav")))
        meta = []
        for path in audio:
            candidate = meta_dir / f"{Path(path).stem}.csv"
            if not candidate.exists():
                raise FileNotFoundError(f"Metadata file not found: {candidate}")
            meta.append(str(candidate))
        return audio, meta

    sony_tr, tau_tr = pair(config.SONY_TRAIN_DIR, config.SONY_TRAIN_META_DIR), pair(config.TAU_TRAIN_DIR, config.TAU_TRAIN_META_DIR)
    sony_te, tau_te = pair(config.SONY_TEST_DIR, config.SONY_TEST_META_DIR), pair(config.TAU_TEST_DIR, config.TAU_TEST_META_DIR)
    return sony_tr[0] + tau_tr[0], sony_tr[1] + tau_tr[1], sony_te[0] + tau_te[0], sony_te[1] + tau_te[1]


# ------------------------------------------------------------------------------------ dataset

class _WindowTable:
    """``dataset.windows`` of the reference is a list of dicts of tensor views (dataset.py:305-311);
    this is the same thing computed on demand from the window start table."""

    def __init__(self, owner):
        self._owner = owner

    def __len__(self):
        return len(self._owner.window_starts)

    def __getitem__(self, idx):
        ds = self._owner
        spec, labels = ds[idx]
        start = int(ds.window_starts[idx])
        return {"spectrogram": spec, "labels": labels, "window_idx": int(idx), "start_frame": start,
                "end_frame": min(start + ds.window_length_frames, ds.total_frames)}


def save_compact_features(path, spec, mask, rot=None):
    """Write one recording's compact features (``rot``: its rotation terms, stored under a third key when given) to ``path``
    so that a concurrent reader sees nothing or the whole file.
    Data-parallel runs construct the dataset on every rank at once: each writer gets its OWN temporary file (same
    directory, so the rename stays on one file system) and renames it into place; the loser of the race replaces the
    winner's file with identical bytes."""
    import os
    import tempfile
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    fd, tmp = tempfile.mkstemp(prefix=path.stem + ".", suffix=".tmp.npz", dir=path.parent)
    try:
        with os.fdopen(fd, "wb") as handle:
            if rot is None:
                np.savez(handle, spec=spec, mask=mask)
            else:
                np.savez(handle, spec=spec, mask=mask, rot=rot)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


class SELDDataset(Dataset):
    """All recordings -> one concatenated timeline -> 5 s windows with 1 s hop (dataset.py:167-330).

    Construction runs entirely on the GPU: each file is uploaded once (int16 when the WAV is 16-bit),
    the fused kernel writes its log-mel frames straight into the shared time-major timeline
    ``spec_tm [total_frames, C, 64]`` and the rasteriser writes the uint16 class mask timeline
    ``mask_tm [total_frames, 648]``; both are cropped per file to min(mel frames, label frames)
    (dataset.py:243-249) and windows are cut across file boundaries like the reference does.
    """

    def __init__(self, audio_files, metadata_files, num_classes=14, device=None, keep_on_device=True,
                 use_gaussian_augmentation=None):
        assert len(audio_files) == len(metadata_files), \
            "Number of audio files must match number of metadata files"
        self._init_fields(num_classes, device)
        if use_gaussian_augmentation is not None:          # smrl_seld_gaussian.py:539-560 (train: True, test: False)
            self.use_gaussian_augmentation = bool(use_gaussian_augmentation)
        self.audio_files = audio_files
        self.metadata_files = metadata_files
        self.keep_on_device = keep_on_device

        logger.info("SELDDataset initialization started...")
        logger.info(f"  Files: {len(audio_files)} audio files")
        logger.info(f"  Grid: {self.I}x{self.J} = {self.total_cells} cells")
        logger.info(f"  Window: {self.window_length_frames} frames, hop {self.hop_length_frames} frames")
        self._build_timeline()
        self._build_window_table()
        logger.info(f"SELDDataset initialized with {len(self)} windows")

    # -- construction -------------------------------------------------------------------------
    def _cache_path(self, audio_path, metadata_path):
        """Where this recording's compact features live under Config.FEATURE_CACHE_DIR, or None (cache off; Gaussian
        label augmentation draws fresh noise per construction, smrl_seld_gaussian.py:397-534, so it is never cached).
        The name carries everything the arrays depend on: both files' size and mtime, the feature set and the signal
        parameters behind it (FFT size, hop, mel bands), the grid, the class count."""
        root = getattr(config, "FEATURE_CACHE_DIR", None)
        if not root or self.use_gaussian_augmentation:
            return None
        import hashlib
        a, m = Path(audio_path), Path(metadata_path)
        sa, sm = a.stat(), m.stat()
        fields = (a.resolve(), sa.st_size, sa.st_mtime_ns, m.resolve(), sm.st_size, sm.st_mtime_ns,
                  getattr(config, "FEATURE_SET", "logmel"), self.I, self.J, self.sample_rate,
                  config.SPECTROGRAM_N_FFT, config.SPECTROGRAM_HOP_LENGTH, config.N_MELS,
                  self.num_classes, getattr(config, "GRID_CELL_DEGREES", 10), "v2")
        if getattr(config, "RESAMPLE_INPUT", False):       # the converter's design is part of what the arrays depend on;
            fields += ("resample-kaiser10.06-zc64-v1",)    # with the switch off the names are the ones they always were
        if getattr(config, "FEATURE_SET", "logmel") == "logmel_nipd":      # what the NIPD channels depend on
            fields += tuple(float(v) for v in _nipd_settings())
        if getattr(self, "pcen_settings", None) is not None:               # Config.PCEN: the log-mel channels hold PCEN values
            fields += ("pcen-v1",) + tuple(self.pcen_settings[k] for k in seld_augment.PCEN_SETTINGS[1:])
        key = "|".join(str(v) for v in fields)
        return Path(root) / f"{a.stem}.{hashlib.sha1(key.encode()).hexdigest()[:16]}.npz"

    def _file_features(self, audio_path, metadata_path):
        """One recording -> (spec_tm [T, C, 64] f32, mask [T, 648] u16, rotation terms [T, 3, 64] f32 or None) on the
        device, cropped to the common frame count (dataset.py:224-249).  With Config.FEATURE_CACHE_DIR they are kept on disk
        in their COMPACT form (1 KB of features + 1.3 KB of label mask per frame; the reference's dense tensors are 37 KB per
        frame) and a later construction uploads them instead of decoding and transforming the recording again.  With
        Config.AUGMENT_ROTATE a cache file without the rotation terms counts as a miss and is replaced."""
        cached = self._cache_path(audio_path, metadata_path)
        if cached is not None and cached.exists():
            with np.load(cached) as z:
                if not self.with_rotation or "rot" in z.files:
                    rot = torch.from_numpy(z["rot"]).to(self.device) if self.with_rotation else None
                    return torch.from_numpy(z["spec"]).to(self.device), torch.from_numpy(z["mask"]).to(self.device), rot
        spec, mask, rot = self._file_features_uncached(audio_path, metadata_path)
        if cached is not None and (rot is not None or not cached.exists()):
            save_compact_features(cached, spec.cpu().numpy(), mask.cpu().numpy(), None if rot is None else rot.cpu().numpy())
        return spec, mask, rot

    def _file_features_uncached(self, audio_path, metadata_path):
        data, rate, bits = _read_wav(audio_path)
        if data.shape[0] != 4 and getattr(config, "FEATURE_SET", "logmel") not in ("logmel_gcc", "logmel_nipd"):
            logger.warning(f"Expected 4 channels but got {data.shape[0]} channels in {audio_path}")
        if bits == 16:
            pcm = torch.from_numpy(data).to(self.device)                       # int16: half the PCIe / HBM bytes
        else:
            pcm = torch.from_numpy(data.astype(np.float32) / float(1 << (bits - 1))).to(self.device)
        return self._features_from_pcm(pcm, rate, _read_metadata_rows(metadata_path))

    def _features_from_pcm(self, pcm, rate, rows):
        signal = pcm
        if int(rate) != self.sample_rate:
            if not getattr(config, "RESAMPLE_INPUT", False):
                raise NotImplementedError(f"sample rate {rate} != {self.sample_rate}: the feature kernel is built for 24 kHz")
            # Config.RESAMPLE_INPUT: polyphase conversion on the device (csrc/resample.hip), fp32 straight into the feature
            # kernels; the labels below keep the FILE's duration, so they do not move
            signal = seld_native.resample(pcm.contiguous(), int(rate), self.sample_rate)
        # [F, C_total, 64]: the reference's per-channel log-mel, optionally followed by the north-star additions
        # (FOA intensity vectors / GCC-PHAT, csrc/spatial.hip; mel-band NIPD, csrc/nipd.hip) as extra input channels
        feature_set = getattr(config, "FEATURE_SET", "logmel")
        if feature_set == "logmel_nipd":
            lo, hi, speed = _nipd_settings()
            spec = seld_native.spatial_features(signal, feature_set, nipd_min_hz=lo, nipd_max_hz=hi, sound_speed=speed)
        else:
            spec = seld_native.spatial_features(signal, feature_set)
        if self.pcen_settings is not None:
            # Config.PCEN (csrc/pcen.hip): the log-mel channels of THIS recording, in place and before
            # the crop -- the smoother restarts per recording, the timeline holds PCEN values; the other channels and the
            # rotation terms are not touched (the switches defined on dB or power values were refused by _init_fields)
            p = self.pcen_settings
            seld_native.pcen(spec, seld_augment.logmel_channels(feature_set, int(spec.shape[1])),
                             seld_native.pcen_coefficient(p["PCEN_TIME_CONSTANT"]), p["PCEN_GAIN"], p["PCEN_BIAS"],
                             p["PCEN_POWER"], p["PCEN_EPS"], out=spec)
        audio_duration = pcm.shape[1] / rate                                   # dataset.py:232 (float64)
        if self.use_gaussian_augmentation:                                      # smrl_seld_gaussian.py:608-618
            mask, _, _ = augment_with_gaussian_mask(rows, audio_duration, self.I, self.J,
                                                    sigma_azimuth=config.GAUSSIAN_SIGMA_AZIMUTH,
                                                    sigma_elevation=config.GAUSSIAN_SIGMA_ELEVATION,
                                                    device=self.device, rng=self._label_rng)
        else:
            mask, _, _ = metadata_to_mask(rows, audio_duration, self.I, self.J, device=self.device)
        frames = min(spec.shape[0], mask.shape[0])                             # dataset.py:243-249
        rot = None
        if self.with_rotation:
            # Config.AUGMENT_ROTATE: the three mel rows per frame the rotating gather needs (csrc/rotate.hip), from the
            # recording's complex STFT -- one recording at a time (a 60 s clip's spectra are 46 MB), freed right after
            seld_augment.check_settings(config, getattr(config, "FEATURE_SET", "logmel"), int(spec.shape[1]))
            rot = seld_native.foa_rotation_terms(seld_native.stft(signal.contiguous()),
                                                 getattr(config, "FOA_CHANNEL_ORDER", "WYZX"))[:frames]
        return spec[:frames], mask[:frames], rot

    def _build_timeline(self):
        specs, masks, rots, rows = [], [], [], []
        for idx, (audio_path, metadata_path) in enumerate(zip(self.audio_files, self.metadata_files)):
            try:
                spec, mask, rot = self._file_features(audio_path, metadata_path)
            except Exception as exc:
                logger.error(f"Error processing file {idx} ({audio_path}): {exc}")
                raise
            specs.append(spec)
            masks.append(mask)
            rots.append(rot)
            rows.append(_read_metadata_rows(metadata_path))
        self._set_segments([int(s.shape[0]) for s in specs], rows)
        self._set_timeline(torch.cat(specs, dim=0), torch.cat(masks, dim=0),
                           torch.cat(rots, dim=0) if self.with_rotation else None)

    def _set_segments(self, frame_counts, rows):
        """Evaluation bookkeeping (seld_eval.py): ``segments`` int64 [n_files, 2] = (first frame, cropped frame count) of
        every file on the timeline; ``metadata_rows`` the files' CSV rows as read, int64 [R, 5] each (not the
        Gaussian-augmented labels)."""
        counts = np.asarray(frame_counts, dtype=np.int64)
        self.segments = np.stack([np.cumsum(counts) - counts, counts], axis=1).reshape(-1, 2)
        self.metadata_rows = [np.asarray(r, dtype=np.int64).reshape(len(r), -1)[:, :5].copy() if len(r)
                              else np.zeros((0, 5), dtype=np.int64) for r in rows]

    def _set_timeline(self, spec_tm, mask_tm, rot_tm=None):
        self.spec_tm = spec_tm.contiguous()            # [total, C, 64] float32 (device)
        self.mask_tm = mask_tm.contiguous()            # [total, 648]  uint16  (device)
        # [total, 3, 64] float32 (device): rotation terms, only when constructed with Config.AUGMENT_ROTATE
        self.rot_tm = rot_tm.contiguous() if rot_tm is not None and self.keep_on_device else None
        self.total_frames = int(self.spec_tm.shape[0])
        self.n_channels = int(self.spec_tm.shape[1])
        # host mirrors for the stock DataLoader path (worker processes must not touch the GPU)
        self._spec_host = self.spec_tm.cpu()
        self._mask_host = self.mask_tm.cpu().numpy()
        if not self.keep_on_device:
            self.spec_tm = self.mask_tm = None
        logger.info(f"Concatenated data: {self.total_frames} total frames, {self.n_channels} channels")

    def _build_window_table(self):
        """dataset.py:271-315: start = 0; while start < total: ...; start += hop."""
        self.window_starts = np.arange(0, self.total_frames, self.hop_length_frames, dtype=np.int64)
        self.windows = _WindowTable(self)
        logger.info(f"Created {len(self.window_starts)} windows")

    @classmethod
    def from_pcm(cls, clips, metadata_rows, sample_rate=24000, num_classes=14, device=None,
                 use_gaussian_augmentation=None):
        """Build from in-memory PCM tensors ([C, L] float32 / int16 each) and parsed metadata rows
        (int [R, 5] each) -- used by the benchmark and the tests, same code path as files."""
        self = cls.__new__(cls)
        SELDDataset._init_fields(self, num_classes, device)
        if use_gaussian_augmentation is not None:
            self.use_gaussian_augmentation = bool(use_gaussian_augmentation)
        specs, masks, rots, kept = [], [], [], []
        for pcm, rows in zip(clips, metadata_rows):
            spec, mask, rot = self._features_from_pcm(pcm.to(self.device), sample_rate, np.asarray(rows))
            specs.append(spec)
            masks.append(mask)
            rots.append(rot)
            kept.append(np.asarray(rows))
        self._set_segments([int(s.shape[0]) for s in specs], kept)
        self._set_timeline(torch.cat(specs, dim=0), torch.cat(masks, dim=0),
                           torch.cat(rots, dim=0) if self.with_rotation else None)
        self._build_window_table()
        return self

    def _init_fields(self, num_classes, device):
        self.audio_files, self.metadata_files = [], []
        self.sample_rate = config.SR
        self.n_fft, self.spectrogram_hop_length, self.n_mels = config.SPECTROGRAM_N_FFT, config.SPECTROGRAM_HOP_LENGTH, config.N_MELS
        self.cell_size_deg = config.GRID_CELL_DEGREES
        self.num_classes = num_classes
        self.I, self.J = int(180 // self.cell_size_deg), int(360 // self.cell_size_deg)
        self.total_cells = self.I * self.J
        self.window_length_samples, self.hop_length_samples = config.WINDOW_LENGTH, config.HOP_LENGTH
        self.window_length_frames = int(self.window_length_samples / self.spectrogram_hop_length)
        self.hop_length_frames = int(self.hop_length_samples / self.spectrogram_hop_length)
        self.device = torch.device(device) if device is not None else _compute_device()
        self.keep_on_device = True
        self._label_rng = np.random.RandomState(config.SEED) if config.SEED is not None else None
        self.use_gaussian_augmentation = bool(config.GAUSSIAN_AUGMENT)
        self.with_rotation = bool(getattr(config, "AUGMENT_ROTATE", False))   # as of construction: decides whether rot_tm exists
        self.rot_tm = None
        # Config.PCEN and its five settings as of construction (seld_augment.pcen_settings), or None: what the log-mel
        # channels of the timeline hold; evaluation compares it with what the checkpoint records
        self.pcen_settings = seld_augment.pcen_settings(config)
        if self.pcen_settings is not None:       # the switches defined on dB or power values: refused before any launch
            seld_augment.check_settings(config, pcen=True)
        # Config.MIC_POSITIONS as of construction: float64 [C, 3], or None (no array: the FOA rules of the augmenting gathers)
        self.mic_array = seld_augment.mic_positions(getattr(config, "MIC_POSITIONS", None))
        self._feature_statistics = None          # statistics of THIS timeline (feature_statistics), computed once
        self.feature_stats = None                # the statistics device_batch applies (set_feature_statistics), or None
        self._feature_scale = self._feature_shift = None
        self._window_class_counts = None         # window_class_counts, computed once

    # -- per-bin standardisation (Config.STANDARDISE_FEATURES; seld_standardise.py) ---------
    def feature_statistics(self):
        """Mean and standard deviation of every (channel, bin) column of this dataset's timeline (seld_standardise
        statistics: CPU tensors), from the device moments kernel (csrc/standardise.hip); computed once and cached.  It sets
        nothing: ``set_feature_statistics`` does."""
        if self._feature_statistics is None:
            if self.spec_tm is None:
                raise RuntimeError("feature_statistics needs the device timeline (keep_on_device=True): the moments are "
                                   "reduced on the GPU, there is no CPU fallback")
            moments = seld_native.feature_moments(self.spec_tm)
            self._feature_statistics = seld_standardise.finalise(moments.cpu(), self.total_frames)
        return self._feature_statistics

    def set_feature_statistics(self, stats):
        """Make ``device_batch`` standardise: every gathered feature becomes fmaf(x, scale[c, f], shift[c, f]) with the
        tables of ``stats`` (seld_standardise statistics, or a checkpoint's ``feature_statistics`` payload), uploaded here
        once.  None switches it off.  ``__getitem__``, the host mirrors and the feature cache stay raw."""
        if stats is None:
            self.feature_stats = self._feature_scale = self._feature_shift = None
            return
        if self.spec_tm is None:
            raise RuntimeError("set_feature_statistics needs the device timeline (keep_on_device=True): the statistics are "
                               "applied by the device window gathers, there is no CPU fallback")
        if "scale" not in stats or "shift" not in stats:
            stats = seld_standardise.from_payload(stats)
        channels = int(stats["mean"].shape[0])
        if channels != self.n_channels:
            raise ValueError(f"feature statistics are for {channels} feature channels, this dataset has {self.n_channels}")
        self.feature_stats = stats
        self._feature_scale = stats["scale"].to(self.spec_tm.device).contiguous()
        self._feature_shift = stats["shift"].to(self.spec_tm.device).contiguous()

    # -- per-window class statistics (Config.BALANCED_SAMPLING; seld_balance.py) -------------
    def window_class_counts(self):
        """int32 [len(self), 16] on the host (numpy): for every window, column c < num_classes = its frames in which class c
        is active somewhere on the grid, column 14 = its frames with any class active, column 15 = its frames inside the
        timeline (tail windows are short).  Reduced from the device-resident label mask by the two kernels of
        csrc/balance.hip -- one pass over ``mask_tm`` -- once, then cached."""
        if getattr(self, "_window_class_counts", None) is None:
            if self.mask_tm is None:
                raise RuntimeError("window_class_counts needs the device timeline (keep_on_device=True): the label mask is "
                                   "reduced on the GPU, there is no CPU fallback")
            frame_mask = seld_native.frame_class_mask(self.mask_tm)
            counts = seld_native.window_class_frames(frame_mask, self.window_length_frames, self.hop_length_frames,
                                                     len(self.window_starts), self.num_classes)
            self._window_class_counts = counts.cpu().numpy()
        return self._window_class_counts

    # -- reference-shaped views ---------------------------------------------------------------
    @property
    def concatenated_spectrograms(self):
        """[C, n_mels, total] view of the timeline (dataset.py:259)."""
        return self._spec_host.permute(1, 2, 0)

    @property
    def concatenated_labels(self):
        """Dense [total, 648, 14] labels (dataset.py:260) -- 36 KB per frame, built on request only."""
        return torch.from_numpy(_expand_mask_host(self._mask_host, self.num_classes))

    # -- Dataset protocol ---------------------------------------------------------------------
    def __len__(self):
        return len(self.window_starts)

    def __getitem__(self, idx):
        """(spec float32 [250, C, 64], labels float32 [250, 648, 14]) as CPU tensors (dataset.py:319-330),
        picklable across DataLoader workers; tail windows are zero / background padded (:282-299)."""
        if idx < 0:
            idx += len(self)
        start = int(self.window_starts[idx])
        w = self.window_length_frames
        n = min(w, self.total_frames - start)
        spec = torch.zeros((w, self.n_channels, self.n_mels), dtype=torch.float32)
        spec[:n] = self._spec_host[start:start + n]
        mask = np.zeros((w, self.total_cells), dtype=np.uint16)
        mask[:n] = self._mask_host[start:start + n]
        return spec, torch.from_numpy(_expand_mask_host(mask, self.num_classes))

    # -- device feed (used by trainer when DEVICE_FEED is on) -----------------------------------
    def device_batch(self, indices, out=None, augment=None, mix=None, spectral=None):
        """Window indices -> (spec [B, 250, C, 64] f32, mask [B, 250, 648] u16) on the device, gathered
        by seld_window_gather straight from the device timeline (no host round trip, no dense labels).
        ``out``: callable (spec_shape, spec_dtype, mask_shape, mask_dtype) -> (spec_buffer, mask_buffer) or None --
        the static input buffers of a captured training step (seld_graph.GraphedTrainStep.static_inputs).
        ``augment``: None, or the windows' parameter table (int32 [B, 12], ``seld_augment.draw``): the batch is then
        produced by the augmenting gathers (csrc/augment.hip) -- channel swap + label cell permutation + masks; on a dataset
        constructed with Config.AUGMENT_ROTATE (``rot_tm`` exists) by the rotating pair (csrc/rotate.hip), which also honours
        the azimuth step in slot [9] of a row.  After ``set_feature_statistics`` all three feature gathers go through their
        standardising exports: affine map after the transform, before the masks.
        ``mix``: None, or the windows' partners (``seld_augment.draw_mix``: partner window index or -1, the partner's spatial
        pattern, its linear power gain): the batch is produced by the mixing pair (csrc/mix.hip) --
        powers added on the stored features, labels united; a window without a partner is the augmenting pair's, bit for
        bit.  Needs ``augment`` rows (identity rows will do); not available on a dataset that holds rotation terms.
        On a dataset constructed with Config.MIC_POSITIONS (``mic_array``) the augmenting pair is the
        array's: 'logmel_gcc' / 'logmel_nipd' features go through the array gather (csrc/micswap.hip), 'logmel' through
        the augmenting gather with the array's channel table, labels through the same cell permutation.  A host row that
        names a pattern which is no symmetry of the array is refused before anything is launched; no ``mix``.
        ``spectral``: None, or the windows' (spectral rows int32 [B, 12], gain curves float32 [B, 64] or None) of
        ``seld_augment.draw_spectral``: frequency shift, gain curve and cutouts, applied by ONE in-place stage on the gathered
        batch (csrc/spectral.hip) whichever of the gathers above produced it.  The order stays
        transform, mix, shift, gain, standardise, masks: the gather runs without masks and without the standardising map, and
        the stage applies both after its own steps.  With identity rows the batch is what it is without ``spectral``, bit
        for bit.  With ``augment`` None the plain gather feeds the stage."""
        if spectral is None:
            return self._gather_batch(indices, out, augment, mix)
        if self.spec_tm is None:
            raise RuntimeError("device_batch needs keep_on_device=True")
        if not (isinstance(spectral, (tuple, list)) and len(spectral) == 2):
            raise ValueError("device_batch: spectral must be (rows, curves) as seld_augment.draw_spectral returns them")
        n, w = len(np.asarray(indices, dtype=np.int64).reshape(-1)), self.window_length_frames
        rows, curves = seld_native.spectral_params(spectral[0], spectral[1], n, w, self.device)   # refused before any launch
        unmasked = params = None
        if augment is not None:                                      # the gather transforms (and mixes); the stage masks
            steps = self.J if getattr(self, "rot_tm", None) is not None else None
            params = seld_native.augment_params(augment, n, w, self.device, steps=steps)      # the rows as they were drawn
            unmasked = augment.clone() if isinstance(augment, torch.Tensor) else np.array(augment, dtype=np.int32)
            unmasked[:, 1:9] = 0
        spec, mask = self._gather_batch(indices, out, unmasked, mix, standardise=False)
        feature_set = getattr(config, "FEATURE_SET", "logmel")
        starts = torch.as_tensor(self.window_starts[np.asarray(indices, dtype=np.int64).reshape(-1)])
        seld_native.window_spectral(spec, starts, int(self.spec_tm.shape[0]), params, rows, curves,
                                    seld_augment.logmel_channels(feature_set, self.n_channels),
                                    seld_augment.freq_mask_channels(feature_set, self.n_channels),
                                    float(getattr(config, "AUGMENT_MASK_VALUE", 0.0)),
                                    scale=getattr(self, "_feature_scale", None), shift=getattr(self, "_feature_shift", None))
        return spec, mask

    def _gather_batch(self, indices, out, augment, mix, standardise=True):
        """``device_batch`` without the spectral stage; ``standardise`` False: the gathers' plain exports although the dataset
        has statistics (the stage applies them)."""
        if self.spec_tm is None:
            raise RuntimeError("device_batch needs keep_on_device=True")
        if mix is not None:
            if augment is None:
                raise ValueError("device_batch: mix needs the windows' augment rows (seld_augment.identity_rows will do)")
            if getattr(self, "rot_tm", None) is not None:
                raise ValueError("device_batch: mixing is not defined together with the rotating gathers (this dataset was "
                                 "constructed with AUGMENT_ROTATE and holds rotation terms)")
        starts = torch.as_tensor(self.window_starts[np.asarray(indices, dtype=np.int64)])
        w = self.window_length_frames
        bufs = None
        if out is not None:
            bufs = out((len(starts), w) + tuple(self.spec_tm.shape[1:]), self.spec_tm.dtype,
                       (len(starts), w) + tuple(self.mask_tm.shape[1:]), self.mask_tm.dtype)
        # set_feature_statistics: the same three gathers through their standardising exports (None: the exports they were)
        scale, shift = getattr(self, "_feature_scale", None), getattr(self, "_feature_shift", None)
        if not standardise:
            scale = shift = None
        if augment is not None:
            table, freq_channels, mask_value = self._augment_tables()
            starts = starts.to(self.device, non_blocking=True)
            if getattr(self, "mic_array", None) is not None:
                if mix is None:
                    return self._mic_batch(starts, w, augment, bufs, scale, shift)
                # mixing on an array is defined without a swap only (check_settings refuses AUGMENT_MIX_PROB together with
                # AUGMENT_SPATIAL): every pattern 0, and the mixing pair below is then what it is without positions
                self._check_mix_on_array(augment, mix)
            if getattr(self, "rot_tm", None) is not None:
                params = seld_native.augment_params(augment, len(starts), w, self.device, steps=self.J)
                spec = seld_native.gather_windows_rotate(self.spec_tm, self.rot_tm, starts, w, params, table,
                                                         getattr(config, "FOA_CHANNEL_ORDER", "WYZX"), self.J, freq_channels,
                                                         mask_value, out=bufs[0] if bufs else None, scale=scale, shift=shift)
                mask = seld_native.gather_windows_permute_rotate(self.mask_tm, starts, w, params, self.I, self.J,
                                                                 out=bufs[1] if bufs else None)
                return spec, mask
            params = seld_native.augment_params(augment, len(starts), w, self.device)     # one more small async copy
            if mix is not None:
                feature_set = getattr(config, "FEATURE_SET", "logmel")
                if not seld_augment.mix_supported(feature_set):
                    raise ValueError(f"device_batch: no mix is defined for FEATURE_SET={feature_set!r}")
                partner, pattern_b, gain = (np.asarray(v).reshape(-1) for v in mix)
                if not len(partner) == len(pattern_b) == len(gain) == len(starts):
                    raise ValueError(f"device_batch: mix must hold one (partner, pattern, gain) per window, {len(starts)} here")
                if len(partner) and (int(partner.min()) < -1 or int(partner.max()) >= len(self.window_starts)):
                    raise ValueError(f"device_batch: mix partner outside -1..{len(self.window_starts) - 1}")
                none = partner < 0
                starts_b = np.where(none, 0, self.window_starts[np.where(none, 0, partner)])
                partners = seld_native.mix_partners(starts_b, pattern_b, np.where(none, np.float32(0), gain), self.device)
                spec = seld_native.gather_windows_mix(self.spec_tm, starts, w, params, partners, table, freq_channels,
                                                      mask_value, seld_augment.mix_iv_channels(feature_set, self.n_channels),
                                                      out=bufs[0] if bufs else None, scale=scale, shift=shift)
                mask = seld_native.gather_windows_mix_mask(self.mask_tm, starts, w, params, partners, self.I, self.J,
                                                           out=bufs[1] if bufs else None)
                return spec, mask
            spec = seld_native.gather_windows_augment(self.spec_tm, starts, w, params, table, freq_channels, mask_value,
                                                      out=bufs[0] if bufs else None, scale=scale, shift=shift)
            mask = seld_native.gather_windows_permute(self.mask_tm, starts, w, params, self.I, self.J,
                                                      out=bufs[1] if bufs else None)
            return spec, mask
        if scale is not None:
            spec = seld_native.gather_windows_affine(self.spec_tm, starts, w, scale, shift, out=bufs[0] if bufs else None)
        else:
            spec = seld_native.gather_windows(self.spec_tm, starts, w, out=bufs[0] if bufs else None)
        mask = seld_native.gather_windows(self.mask_tm, starts, w, out=bufs[1] if bufs else None)
        return spec, mask

    def _check_mix_on_array(self, augment, mix):
        """``device_batch(augment=..., mix=...)`` on a dataset that knows its microphone array: host rows and partner patterns
        must all be the identity (a device-resident parameter table is trusted, as everywhere)."""
        if not (isinstance(augment, torch.Tensor) and augment.is_cuda):
            rows = np.asarray(torch.as_tensor(augment))
            if rows.ndim == 2 and rows.shape[1] >= 1 and rows[:, 0].any():
                raise ValueError("device_batch: mixing on a microphone array (this dataset was constructed with MIC_POSITIONS) "
                                 "is defined without a channel swap only: every window's spatial pattern must be 0")
        if len(mix) == 3 and np.asarray(mix[1]).any():
            raise ValueError("device_batch: mixing on a microphone array (this dataset was constructed with MIC_POSITIONS) is "
                             "defined without a channel swap only: every partner's spatial pattern must be 0")

    def _mic_batch(self, starts, w, augment, bufs, scale, shift):
        """``device_batch`` with ``augment`` rows and no ``mix`` on a dataset that knows its microphone array (DESIGN.md
        section 25)."""
        if getattr(self, "rot_tm", None) is not None:
            raise ValueError("device_batch: no rotation is defined for a microphone array (this dataset was constructed with "
                             "MIC_POSITIONS)")
        feature_set = getattr(config, "FEATURE_SET", "logmel")
        key = (feature_set, self.n_channels)
        if getattr(self, "_mic_key", None) != key:
            seld_augment.check_settings(config, feature_set, self.n_channels, array=self.mic_array)
            self._mic_perm = seld_augment.mic_permutations(self.mic_array)
            self._mic_table = seld_augment.mic_channel_table(self.mic_array)
            self._mic_freq_channels = seld_augment.freq_mask_channels(feature_set, self.n_channels)
            self._mic_key = key
        if not (isinstance(augment, torch.Tensor) and augment.is_cuda):     # (a device table is trusted: no synchronise; the
            patterns = np.asarray(torch.as_tensor(augment))[:, 0]           #  kernel writes its bad rows untransformed)
            known = (patterns >= 0) & (patterns < seld_augment.PATTERNS)
            bad = sorted({int(p) for p in patterns[known] if self._mic_perm[int(p), 0] < 0})
            if bad:
                valid = [int(p) for p in np.flatnonzero(self._mic_perm[:, 0] >= 0)]
                raise ValueError(f"device_batch: spatial patterns {bad} are no symmetries of this microphone array (valid: "
                                 f"{valid}): the features would stay put while the labels move")
        params = seld_native.augment_params(augment, len(starts), w, self.device)
        mask_value = float(getattr(config, "AUGMENT_MASK_VALUE", 0.0))
        if feature_set == "logmel":
            spec = seld_native.gather_windows_augment(self.spec_tm, starts, w, params, self._mic_table,
                                                      self._mic_freq_channels, mask_value, out=bufs[0] if bufs else None,
                                                      scale=scale, shift=shift)
        else:
            spec = seld_native.gather_windows_mic(self.spec_tm, starts, w, params, self._mic_perm, feature_set,
                                                  self._mic_freq_channels, mask_value, out=bufs[0] if bufs else None,
                                                  scale=scale, shift=shift)
        mask = seld_native.gather_windows_permute(self.mask_tm, starts, w, params, self.I, self.J,
                                                  out=bufs[1] if bufs else None)
        return spec, mask

    def _augment_tables(self):
        """(channel table uint8 [16, C], channels that take frequency masks, mask value) for this dataset's feature set and
        Config.FOA_CHANNEL_ORDER; a feature set without a defined channel swap gets identity rows."""
        feature_set = getattr(config, "FEATURE_SET", "logmel")
        order = getattr(config, "FOA_CHANNEL_ORDER", "WYZX")
        key = (feature_set, order, self.n_channels)
        if getattr(self, "_augment_key", None) != key:
            self._augment_key = key
            self._augment_table = (seld_augment.channel_table(feature_set, self.n_channels, order),
                                   seld_augment.freq_mask_channels(feature_set, self.n_channels))
        return self._augment_table + (float(getattr(config, "AUGMENT_MASK_VALUE", 0.0)),)


def _expand_mask_host(mask, num_classes):
    """Host-side expansion for the stock DataLoader path: uint16 [..., G] -> float32 [..., G, M] with the
    reference's background rule (dataset.py:110-117).  Pure indexing, no arithmetic."""
    bits = (mask[..., None] >> np.arange(num_classes, dtype=np.uint16)) & np.uint16(1)
    dense = bits.astype(np.float32)
    dense[..., num_classes - 1][mask == 0] = 1.0
    return dense
