"""Inference CLI: recordings -> SELD event CSVs, one per recording (no reference counterpart).

    python infer.py --checkpoint best_model.pth --out-dir DIR [--tta all | --tta 0,2,9] [--track] [--refine] [--resample]
                    [--thresholds thresholds.json] a.wav [b.wav ...]

Each recording becomes a one-segment timeline (features through the dataset's own path, no metadata rows), its 5 s
windows run through the checkpoint's model in timeline order, and the decoded events are written to DIR/<stem>.csv as
``meta_frame,class,rank,azimuth,elevation`` rows -- the metadata format the dataset reads.  With ``--track`` the
detections are linked into tracks first: the third column is the track id, and DIR/<stem>.tracks.csv
lists ``class,track,onset_m,offset_m,detected_frames`` of every kept track.  With ``--refine`` azimuth and elevation are the
nearest integer degrees of the detections' sub-cell directions, not the centres of their 10-degree cells.
With ``--resample`` a recording whose rate is not 24 kHz is converted on the GPU first.
With ``--thresholds`` the per-class detection thresholds of a sweep's thresholds file take the place of ``--threshold``
(DESIGN.md section 17).
A checkpoint trained with FEATURE_SET 'logmel_nipd' carries NIPD_MIN_HZ, NIPD_MAX_HZ and SOUND_SPEED in its ``config``: the
recordings' features are computed with those values, which are logged.
A checkpoint trained with Config.PCEN carries the switch and its five settings the same way: the recordings' log-mel
channels are normalised with them, and Config is put back afterwards.
"""
import argparse
import logging
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import dataset  # noqa: E402
import seld_augment  # noqa: E402
import seld_eval  # noqa: E402
import trainer  # noqa: E402
from utils import safe_torch_load  # noqa: E402


def parse_args(argv=None):
    cfg = trainer.config
    p = argparse.ArgumentParser(description="Decode SELD events from WAV recordings with a trained checkpoint.")
    p.add_argument("--checkpoint", required=True, help="checkpoint written by train_model (e.g. best_model.pth)")
    p.add_argument("--out-dir", required=True, help="directory for the event CSVs")
    p.add_argument("--model-type", default=None, help="model kind; default: the checkpoint's Config, else Config.MODEL_TYPE")
    p.add_argument("--batch-size", type=int, default=cfg.BATCH_SIZE)
    p.add_argument("--threshold", type=float, default=cfg.SELD_THRESHOLD)
    p.add_argument("--thresholds", default=None,
                   help="thresholds file written by a sweep (evaluate_seld(..., thresholds_out=FILE)): its per-class "
                        "detection thresholds are applied; wins over --threshold")
    p.add_argument("--max-peaks", type=int, default=cfg.SELD_MAX_PEAKS)
    p.add_argument("--tta", default=None,
                   help="test-time augmentation: 'all' or spatial patterns such as 0,2,9 whose un-permuted grid maps are "
                        "averaged (one forward per pattern; default: Config.SELD_TTA_PATTERNS)")
    p.add_argument("--track", action=argparse.BooleanOptionalAction, default=bool(getattr(cfg, "SELD_TRACK", False)),
                   help="link the detections into tracks: CSV column 3 becomes a track id, <stem>.tracks.csv lists the tracks "
                        "(default: Config.SELD_TRACK; --no-track switches it off)")
    p.add_argument("--track-gate-deg", type=float, default=cfg.SELD_TRACK_GATE_DEG,
                   help="a detection continues a track within this angle of its last cell")
    p.add_argument("--track-max-gap", type=int, default=cfg.SELD_TRACK_MAX_GAP,
                   help="meta-frames a track survives without a detection (filled), 0..16")
    p.add_argument("--track-min-len", type=int, default=cfg.SELD_TRACK_MIN_LEN,
                   help="tracks spanning fewer meta-frames are removed")
    p.add_argument("--refine", action=argparse.BooleanOptionalAction, default=bool(getattr(cfg, "SELD_REFINE", False)),
                   help="write sub-cell directions (integer degrees) in place of the 10-degree cell centres "
                        "(default: Config.SELD_REFINE; --no-refine switches it off)")
    p.add_argument("--resample", action=argparse.BooleanOptionalAction, default=bool(getattr(cfg, "RESAMPLE_INPUT", False)),
                   help="convert recordings whose rate is not 24 kHz (48 kHz, 44.1 kHz, ...) on the GPU first "
                        "(default: Config.RESAMPLE_INPUT; --no-resample: such a recording is an error)")
    p.add_argument("--device", default=None, help="default: the current ROCm device")
    p.add_argument("--use-ema", action="store_true",
                   help="load the checkpoint's ema_state_dict (default: Config.EVAL_USE_EMA); an error when it has none")
    p.add_argument("wavs", nargs="+", help="PCM WAV recordings: 24 kHz, or with --resample any rate the converter covers "
                                             "(8, 11.025, 12, 16, 22.05, 32, 44.1, 48, 88.2, 96, 192 kHz)")
    return p.parse_args(argv)


def _pcm(path):
    data, rate, bits = dataset._read_wav(path)
    if bits == 16:
        return torch.from_numpy(data), rate                     # int16 straight into the feature kernel
    return torch.from_numpy(data.astype(np.float32) / float(1 << (bits - 1))), rate


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    device = torch.device(args.device) if args.device else dataset._compute_device()
    checkpoint = safe_torch_load(args.checkpoint, map_location=device)
    model_type = args.model_type or getattr(checkpoint.get("config"), "MODEL_TYPE", None)
    if model_type:
        trainer.config.MODEL_TYPE = model_type
    # FEATURE_SET 'logmel_nipd': the range and the speed of sound the checkpoint's features were computed with
    own = getattr(checkpoint.get("config"), "__dict__", {})
    nipd = {k: float(own[k]) for k in trainer.NIPD_SETTINGS if k in own}
    if nipd:
        logging.getLogger(__name__).info("NIPD settings of the checkpoint: " + ", ".join(f"{k} = {v:g}" for k, v in nipd.items()))
    # Config.PCEN and its five settings travel the same way: the recordings' log-mel channels are
    # normalised with what the weights were trained on
    pcen = {k: own[k] for k in trainer.PCEN_SETTINGS if k in own}
    if pcen.get("PCEN"):
        logging.getLogger(__name__).info("PCEN settings of the checkpoint: "
                                         + ", ".join(f"{k} = {v:g}" for k, v in pcen.items() if k != "PCEN"))
    # a microphone array's geometry (Config.MIC_POSITIONS) travels in the checkpoint like the NIPD settings
    array = seld_augment.mic_positions(own.get("MIC_POSITIONS", getattr(trainer.config, "MIC_POSITIONS", None)))
    patterns = seld_augment.tta_patterns(getattr(trainer.config, "SELD_TTA_PATTERNS", ()) if args.tta is None else args.tta,
                                         array=array)
    track = {"gate_deg": args.track_gate_deg, "max_gap": args.track_max_gap, "min_len": args.track_min_len} \
        if args.track else False
    per_class = None
    if args.thresholds:
        per_class = seld_eval.load_thresholds(args.thresholds, max_peaks=args.max_peaks, tta_patterns=patterns,
                                              refine=args.refine)["per_class"]
    model = None
    written = []
    for wav in args.wavs:
        pcm, rate = _pcm(wav)
        saved = dataset.config.RESAMPLE_INPUT
        dataset.config.RESAMPLE_INPUT = bool(args.resample)      # the switch the dataset path reads, for this run only
        saved_nipd = {k: getattr(dataset.config, k) for k in nipd}
        for k, v in nipd.items():
            setattr(dataset.config, k, v)
        saved_pcen = {k: vars(dataset.config)[k] for k in pcen if k in vars(dataset.config)}
        for k, v in pcen.items():
            setattr(dataset.config, k, v)
        own_array = "MIC_POSITIONS" in vars(dataset.config)      # (restored below without leaving an instance attribute)
        saved_array = vars(dataset.config).get("MIC_POSITIONS")
        dataset.config.MIC_POSITIONS = array
        try:
            ds = dataset.SELDDataset.from_pcm([pcm], [np.zeros((0, 5), dtype=np.int64)], sample_rate=rate, device=device,
                                              use_gaussian_augmentation=False)
        finally:
            dataset.config.RESAMPLE_INPUT = saved
            for k, v in saved_nipd.items():
                setattr(dataset.config, k, v)
            for k in pcen:                                       # likewise: no instance attribute is left behind
                if k in saved_pcen:
                    setattr(dataset.config, k, saved_pcen[k])
                else:
                    delattr(dataset.config, k)
            if own_array:
                dataset.config.MIC_POSITIONS = saved_array
            else:
                del dataset.config.MIC_POSITIONS
        trainer.check_dataset_pcen(trainer.checkpoint_pcen_settings(checkpoint), ds, "the checkpoint records")
        seld_augment.check_tta(patterns, getattr(trainer.config, "FEATURE_SET", "logmel"), ds.n_channels, array=array)
        # a checkpoint trained on standardised features carries their statistics: the recording's gathers apply them
        # (Config.STANDARDISE_FEATURES on and none in the checkpoint: an error, as in evaluate_seld)
        trainer.apply_checkpoint_statistics(checkpoint, ds)
        if model is None:
            model = trainer.prepare_model_for_device(trainer.build_model((ds.I, ds.J), True, n_channels=ds.n_channels),
                                                     device)
            model.load_state_dict(trainer.select_state_dict(checkpoint, True if args.use_ema else None))
            model.eval()
        result = seld_eval.evaluate_logits(trainer.timeline_logits(model, ds, args.batch_size, device, patterns=patterns),
                                           ds, threshold=None if per_class else args.threshold, max_peaks=args.max_peaks,
                                           events_dir=args.out_dir, names=[Path(wav).stem], patterns=patterns, track=track,
                                           refine=args.refine, sweep=(), class_thresholds=per_class)
        path = result["event_files"][0]
        written.append(path)
        if result["tracking"]:
            print(f"{wav}: {result['FP']} events of {result['tracking']['tracks_kept']} tracks -> {path}, "
                  f"{result['track_files'][0]}")
        else:
            print(f"{wav}: {result['FP']} events -> {path}")
    return written


if __name__ == "__main__":
    main()
