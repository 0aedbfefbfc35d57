"""Configuration surface of the SELD training path (drop-in for the reference's ``config.py``).

Every attribute the reference defines (config.py:7-97) is present with the same name, type and
default, and ``Config()`` creates the output / checkpoint directories and the derived dataset
paths exactly like config.py:99-118 (main.py and trainer.py rely on CHECKPOINT_PATH existing).
Attributes below the "MI355X additions" line do not exist upstream; they default to values that
keep upstream semantics on a CPU and switch the GPU fast paths on when a ROCm device is used.
"""
from pathlib import Path

_SR = 24000


class Config:
    # ---- locations (relative to this file, like the reference) ---------------------------
    BASE_PATH = Path(__file__).parent
    AUDIO_PATH = BASE_PATH / "foa_dev"
    METADATA_PATH = BASE_PATH / "metadata_dev"
    OUTPUT_PATH = BASE_PATH / "outputs"
    CHECKPOINT_PATH = BASE_PATH / "checkpoints"

    # ---- data selection -----------------------------------------------------------------
    USE_FULL_DATASET = True
    TRAIN_AUDIO_FILE = "fold3_room21_mix001.wav"
    TRAIN_META_FILE = "fold3_room21_mix001.csv"
    TEST_AUDIO_FILE = "fold4_room23_mix001.wav"
    TEST_META_FILE = "fold4_room23_mix001.csv"

    STARSS22_CLASSES = dict(enumerate((
        "Female speech, woman speaking", "Male speech, man speaking", "Clapping", "Telephone",
        "Laughter", "Domestic sounds", "Walk, footsteps", "Door, open or close", "Music",
        "Musical instrument", "Water tap, faucet", "Bell", "Knock", "Background")))

    # ---- model ---------------------------------------------------------------------------
    MODEL_TYPE = "resnet_conformer"      # 'cnn' | 'crnn' | 'conformer' | 'resnet_conformer'
    NUM_CLASSES = 14
    N_CHANNELS = 4

    CRNN_CNN_CHANNELS = [64, 128, 256, 512]
    CRNN_RNN_HIDDEN = 256
    CRNN_RNN_LAYERS = 2
    CRNN_DROPOUT = 0.3

    CONF_D_MODEL = 256
    CONF_N_HEADS = 4
    CONF_N_LAYERS = 2
    CONF_KERNEL_SIZE = 31
    CONF_DROPOUT = 0.3

    RESNET_CONF_D_MODEL = 512
    RESNET_CONF_N_HEADS = 8
    RESNET_CONF_N_LAYERS = 4
    RESNET_DROPOUT = 0.3

    # ---- optimisation --------------------------------------------------------------------
    NUM_EPOCHS = 30
    BATCH_SIZE = 16
    LEARNING_RATE = 1e-3
    LR_DECAY_FACTOR = 0.5
    LR_DECAY_PATIENCE = 5
    WEIGHT_DECAY = 1e-4

    LOSS_TYPE = "mse"                    # 'mse' | 'ce'
    W_CLASS = 1.0
    W_AIUR = 1.0
    W_CL = 1.0

    PATIENCE = 20
    MIN_DELTA = 1e-4

    SAVE_EVERY_N_EPOCHS = 5
    KEEP_LAST_N_CHECKPOINTS = 3

    # ---- signal processing: 40 ms frames, 20 ms hop at 24 kHz ------------------------------
    SPECTROGRAM_N_FFT = int(0.04 * _SR)          # 960
    SPECTROGRAM_HOP_LENGTH = int(0.02 * _SR)     # 480
    N_MELS = 64
    SR = _SR

    # ---- windowing of the concatenated timeline: 5 s windows, 1 s hop ----------------------
    WINDOW_LENGTH = int(5 * _SR)                 # 120000 samples = 250 frames
    HOP_LENGTH = int(1 * _SR)                    # 24000 samples  = 50 frames

    # ---- DOA grid ------------------------------------------------------------------------
    I = None
    J = None
    GRID_CELL_DEGREES = 10

    # ==== MI355X additions (not in the reference) ==========================================
    AMP_DTYPE = "bf16"          # autocast dtype on ROCm devices: 'bf16' or 'fp32'
    CHANNELS_LAST = True        # NHWC conv blocks (MIOpen/hipBLASLt MFMA path)
    FUSED_LOSS = True           # seld_softmax_mse / seld_softmax_ce instead of softmax + mse_loss / cross_entropy + autograd
    CE_FOCAL_GAMMA = 0.0        # LOSS_TYPE 'ce': 0 = the reference's weighted cross-entropy; >= 1 multiplies every cell's term
                                # by (summed probability of the classes other than its target)^gamma, which takes weight off
                                # the ~97 % of grid cells that are easy background (values in (0, 1) are refused)
    FUSED_CONV_TAIL = True      # BatchNorm -> ReLU -> MaxPool of the CNN blocks in two HBM passes (csrc/convtail.hip)
    CONV_DGRAD_AS_FORWARD = True  # encoder 3x3 convs: data gradient as a forward conv with transposed, flipped weights
    FUSED_CONV_WGRAD = True     # encoder 3x3 convs: weight gradient by the HIP split-K MFMA kernel (csrc/convwgrad.hip),
                                # written straight into the parameter's gradient; shapes it does not cover: the library.
                                # Part of the _Conv3x3 path: no effect when CONV_DGRAD_AS_FORWARD is off
    FUSED_CONV_DGRAD = True     # encoder 3x3 convs: data gradient by the HIP MFMA kernel (csrc/convdgrad.hip) from the weights
                                # where they lie (no flip / transpose launch, no library call); shapes it does not cover:
                                # the library.  Part of the _Conv3x3 path: no effect when CONV_DGRAD_AS_FORWARD is off
    FUSED_CONV_FWD = True       # encoder 3x3 convs in training: forward by the HIP MFMA kernel on the data-gradient loop
                                # (csrc/convfwd.hip), which also forms the BatchNorm sums, so the tail runs without its
                                # statistics pass; blocks on model_crnn.ConvBlock.fused_fwd_adopted only.  Part of the _Conv3x3
                                # path and needs FUSED_CONV_TAIL; eval, fp32 and other shapes: the library
    FUSED_FIRST_BLOCK = True    # encoder block 1 (4 -> 64 channels, bf16 training): the 36-MAC convolution is recomputed inside
                                # the BatchNorm / ReLU / pool kernels and inside its own weight gradient instead of stored
                                # (csrc/convfirst.hip): its 65.5 MB output and gradient never reach HBM.  Needs FUSED_CONV_TAIL
                                # and CONV_DGRAD_AS_FORWARD; other shapes, fp32 and eval keep the general path
    FUSED_DWCONV = "auto"       # channels-last Conformer conv module with the HIP depthwise Conv1d (csrc/dwconv.hip):
                                # fewer GPU microseconds but more host work; "auto" = always under GRAPH_STEP (no host work
                                # per iteration), else modules with d_model >= 512 (eager: +3 % on the ResNet50-Conformer,
                                # -7 % on the host-bound d_model-256 Conformer)
    CONV1X1_AS_GEMM = True      # ResNet bottlenecks: the 1x1 / stride-1 convolutions as GEMMs on the channels-last rows
                                # (hipBLASLt forward / data gradient, split-K weight gradient) instead of MIOpen's
    FUSED_QKV = True            # Conformer self-attention: the q / k / v projections of the same input as ONE GEMM on packed
                                # parameters (seld_pack.py), forward and backward
    FUSED_LAYERNORM = True      # head: LayerNorm -> ReLU in one kernel, activations stay bf16 (csrc/layernorm.hip)
    OVERLAP_WEIGHT_GRADS = True  # CRNN: weight gradients of the head and of GRU layer 1 on a side HIP stream, under the
                                # backward recurrences that occupy 16 of the 256 CUs (seld_overlap.py)
    FUSED_GRU = True            # persistent BiGRU kernel instead of MIOpen's per-step GEMMs
    DEVICE_FEED = True          # train from device-resident features / compact labels (no 290 MB/step H2D)
    MASTER_WEIGHTS = True       # bf16 runs: the conv / Linear / GRU weight matrices live in the model as bf16 working
                                # copies of fp32 masters owned by the optimiser (same values autocast would cast to
                                # every iteration, without ~40-340 cast kernels per iteration; bf16 gradient all-reduce)
    FUSED_ADAM_KERNEL = True    # master-weight mode, captured steps: the whole Adam update incl. the bf16 gradient read and the
                                # bf16 working-copy write as one multi-tensor launch (csrc/adam.hip) instead of cast + the
                                # framework's fused Adam + cast
    GRAPH_STEP = True           # one optimiser iteration = one replayed HIP graph per input shape (seld_graph.py): the eager
                                # loop spends ~3.5 ms of host time enqueueing ~300 launches per CRNN iteration; data
                                # parallel: one graph per backward stage, gradient buckets all-reduced in between
                                # (OVERLAP_ALLREDUCE below), then the update graph
    OVERLAP_ALLREDUCE = True    # data parallel + GRAPH_STEP: the backward pass is cut at the models' seld_cut.boundary points and
                                # captured as one graph per stage; the gradients a stage completes are all-reduced (RCCL,
                                # asynchronously) while the next stages run.  False: one graph, then one blocking exchange
    ALLREDUCE_CUT_LEVELS = 2    # 1: cut the backward pass only between the recurrent / attention part and the encoder; 2: also
                                # before the encoder's last block (one more bucket under way, ~50 us more per iteration:
                                # tools/bench_stages.py measured 3.62 ms as one graph, 3.67 / 3.72 / 3.77 ms with 0 / 1 / 2 cuts)
    GRAD_REDUCE_DTYPE = "param"  # wire dtype of that exchange: "param" = the bf16 working-weight gradients are summed in bf16
                                # (half the xGMI bytes), "fp32" = cast into fp32 buffers first (what an autocast port of the
                                # reference would reduce; the buffers double as the fp32 masters' gradients)
    TUNED_GEMMS = True          # apply tuned/gemm_gfx950.csv: hipBLASLt / rocBLAS kernel selections for the models' GEMM
                                # shapes, timed offline on an MI355X (seld_tuned.py; ignored on any other library stack)
    DDP_BUCKET_MB = 8           # RCCL all-reduce bucket size: with bf16 working weights the CRNN's gradients are 22 MB, so
                                # 8 MB gives three buckets -- the head's (ready first) reduces under the GRU / conv backward
    SYNC_BATCHNORM = False      # per-rank BN statistics by default
    SEED = None                 # the reference never seeds; set an int for reproducible runs
    FEATURE_SET = "logmel"      # 'logmel' (the reference) | 'logmel_iv' (FOA: + 3 intensity-vector channels) |
                                # 'logmel_gcc' (MIC array: + C(C-1)/2 GCC-PHAT channels) | 'logmel_nipd' (MIC array: + C-1
                                # mel-band NIPD channels against channel 0, csrc/nipd.hip); the
                                # model's n_channels follows the dataset (4 -> 7, 8 -> 36, 8 -> 15)
    NIPD_MIN_HZ = 50.0          # 'logmel_nipd': STFT bins below this carry no usable phase (the 1 / f of the weights blows
                                # their noise up); mel bands without a bin in [NIPD_MIN_HZ, NIPD_MAX_HZ] are exactly 0
    NIPD_MAX_HZ = 2000.0        # should be c / (2 * largest microphone spacing), the spatial-aliasing limit above which a
                                # phase difference wraps; 2 kHz is SALSA-Lite's value for a 4.2 cm array
    SOUND_SPEED = 343.0         # m/s: scales the NIPD channels to metres of extra path length (c * delay)
    FEATURE_CACHE_DIR = None    # directory for the per-recording COMPACT features (fp32 log-mel [T,C,64] + uint16 label mask
                                # [T,648], 2.3 KB per frame): a later SELDDataset construction uploads them instead of
                                # decoding and transforming the recording again
    THREE_TERM_LOSS = False     # total = W_CLASS * class + W_AIUR * AIUR + W_CL * CL on probabilities, as
                                # smrl_seld_gaussian.py:1058-1072 (BASELINE configs[4]: with GAUSSIAN_AUGMENT and the
                                # ResNet50-Conformer); False = the modular loss.py, class term only (loss.py:158-166)
    GAUSSIAN_AUGMENT = False    # smrl_seld_gaussian.py:397-534 label augmentation (+-2 sigma box per source)
    GAUSSIAN_SIGMA_AZIMUTH = 5.0
    GAUSSIAN_SIGMA_ELEVATION = 5.0
    # Training augmentation inside the device window gather (seld_augment.py, csrc/augment.hip).  All
    # off by default; applied to the training feed only, never to evaluation / inference.  Needs DEVICE_FEED (the host
    # DataLoader path refuses to run with a switch on: there is no CPU fallback)
    AUGMENT_SPATIAL = False     # FOA audio channel swapping: one of the 16 sign-and-swap transforms per window and epoch, DOA
                                # labels moved to match ('logmel' with 4 channels and 'logmel_iv' only)
    AUGMENT_ROTATE = False      # rotation about the vertical axis in steps of one grid cell (10 degrees) on top of mirror and
                                # elevation flip: 144 transforms instead of 16 (csrc/rotate.hip).  Implies the
                                # spatial draw; needs DEVICE_FEED and a dataset constructed with the switch on (three extra mel
                                # rows per frame of the timeline); 'logmel' with 4 channels and 'logmel_iv' only
    AUGMENT_TIME_MASKS = 0      # SpecAugment: time masks per window, 0..2, every channel
    AUGMENT_TIME_MASK_MAX = 0   # longest time mask in frames (a length is uniform in [0, max])
    AUGMENT_FREQ_MASKS = 0      # frequency masks per window, 0..2, log-mel, intensity-vector and NIPD channels (not GCC-PHAT lags)
    AUGMENT_FREQ_MASK_MAX = 0   # widest frequency mask in mel bins
    AUGMENT_MASK_VALUE = 0.0    # what masked elements are set to (0.0 = what tail windows are padded with)
    AUGMENT_MIX_PROB = 0.0      # probability that a training window is mixed with a partner window of the timeline, labels
                                # united (csrc/mix.hip): powers add on the stored features.  'logmel' and
                                # 'logmel_iv' only; not together with AUGMENT_ROTATE
    AUGMENT_MIX_GAIN_DB = 6.0   # the partner's level relative to the window: uniform in +- this many dB
    # One in-place stage on the gathered batch (csrc/spectral.hip), after any of the gathers above and
    # before standardisation and masks; every feature set; all off by default (then no launch is added)
    AUGMENT_FREQ_SHIFT_MAX = 0  # frequency shifting: the window moved by s mel bands, s uniform in [-max, max] (<= 63), the edge
                                # band replicated; mel-axis channels only (not GCC-PHAT lags)
    AUGMENT_LEVEL_DB = 0.0      # a random overall level per window, uniform in +- this many dB, added to the log-mel channels
    AUGMENT_FILTER_PROB = 0.0   # FilterAugment: probability that a window gets a random piecewise gain curve over the mel bands
    AUGMENT_FILTER_DB = 6.0     # its gains: uniform in +- this many dB
    AUGMENT_FILTER_BANDS = (3, 6)   # its number of bands: uniform in [fewest, most]
    AUGMENT_FILTER_TYPE = "linear"  # 'linear' (a gain per band edge, interpolated) or 'step' (a gain per band)
    AUGMENT_CUTOUTS = 0         # random cutout: time x frequency rectangles per window, 0..2, set to AUGMENT_MASK_VALUE on the
                                # mel-axis channels
    AUGMENT_CUTOUT_TIME_MAX = 0 # longest cutout in frames (a length is uniform in [0, max])
    AUGMENT_CUTOUT_FREQ_MAX = 0 # widest cutout in mel bins
    FOA_CHANNEL_ORDER = "WYZX"  # which input channel is which: 'WYZX' (STARSS / DCASE FOA recordings) or 'WXYZ'
    MIC_POSITIONS = None        # microphone-array recordings: the microphone positions, which define the array's channel swaps
                                # (seld_augment.py, csrc/micswap.hip).  None = unknown (FOA rules: an
                                # array gets masks only), the preset "tetra_starss" (the STARSS22 tetrahedron, 4.2 cm), or C
                                # rows of (x, y, z) in metres, x towards azimuth 0, y towards azimuth +90, z up.  With them
                                # AUGMENT_SPATIAL and SELD_TTA_PATTERNS work on 'logmel', 'logmel_gcc' and 'logmel_nipd' over
                                # the patterns that map the array onto itself ("all" = those); saved in the checkpoint
    # Per-bin feature standardisation inside the device window gathers (seld_standardise.py, csrc/standardise.hip; DESIGN.md
    # section 22).  Off by default: every entry point, checkpoint and benchmark figure is then what it was
    STANDARDISE_FEATURES = False  # train_model reduces mean / std of every (channel, mel bin or lag) over the TRAINING timeline
                                # on the device, both datasets' gathers then write (x - mean) / std -- after the augmentation
                                # transform, before the SpecAugment masks -- and every checkpoint carries the statistics under
                                # 'feature_statistics'; test_model / evaluate_seld / infer.py apply a checkpoint's statistics
                                # whenever it holds them (with the switch on and none in the checkpoint: an error).  Needs
                                # DEVICE_FEED like the augmentation switches (the host DataLoader path refuses to run)
    # Per-channel energy normalisation of the log-mel channels (csrc/pcen.hip).  Off by default: every
    # entry point, cache file name, checkpoint and benchmark figure is then what it was
    PCEN = False                # SELDDataset replaces each recording's log-mel channels (dB) by
                                # y = (E (eps + M)^-gain + bias)^power - bias^power, E the mel power and M its first-order
                                # average along time, restarted per recording: nearly independent of the recording level,
                                # stationary background suppressed.  The other channels (intensity vectors, GCC-PHAT, NIPD)
                                # stay.  Not with the switches defined on dB or power values (AUGMENT_MIX_PROB,
                                # AUGMENT_ROTATE, AUGMENT_LEVEL_DB, AUGMENT_FILTER_PROB); needs the device path (the host
                                # DataLoader path refuses to run); the five settings travel in the checkpoint
    PCEN_TIME_CONSTANT = 0.4    # seconds: the smoother's time constant (seld_native.pcen_coefficient turns it into s)
    PCEN_GAIN = 0.98            # alpha in [0, 1]: how much of the smoothed level is divided out
    PCEN_BIAS = 2.0             # delta > 0: added before the root
    PCEN_POWER = 0.5            # r in (0, 1]: the root
    PCEN_EPS = 1e-10            # the log-mel's own power floor (-100 dB).  librosa's default of 1e-6 presumes magnitudes of
                                # integer-scaled samples (x 2^31); the mel powers here come from samples in [-1, 1)
    # Class-balanced window sampling of the training feed (seld_balance.py, csrc/balance.hip).  Off by
    # default: every entry point, epoch order, checkpoint and benchmark figure is then what it was
    BALANCED_SAMPLING = False   # the training feed draws each epoch's len(dataset) windows WITH replacement, weighted by the
                                # classes each window holds (reduced once from the device-resident label mask); epoch length,
                                # steps per epoch and the LR schedule do not move.  Evaluation, test_model, infer.py and the
                                # test loader are untouched.  Needs DEVICE_FEED like the augmentation switches (the host
                                # DataLoader path refuses to run); every rank reproduces the same order from (SEED, epoch)
    BALANCE_POWER = 1.0         # beta in [0, 1]: an active window weighs max over its classes of (windows holding the
                                # class)^-beta.  0 = all active windows alike (only the silent share is controlled), 1 = a
                                # window is weighted by its rarest class (classes that never share a window are then expected
                                # in equally many drawn windows)
    BALANCE_SILENT_SHARE = None # expected share of the draws that go to windows without any class, in [0, 1): None = their
                                # natural share, 0 = never drawn
    BALANCE_MIN_FRAMES = 5      # a class is present in a window from this many 20 ms frames on (5 = one 100 ms label frame)
    # Guarded optimiser update (csrc/guard.hip, csrc/adam.hip).  All off by default; device-side, inside
    # the one-launch update, so they need the master-weight path (bf16 autocast on a ROCm device): make_optimizer refuses
    # a switched-on guard anywhere else
    GRAD_CLIP_NORM = 0.0        # > 0: scale the gradients so that their global L2 norm is at most this (clip_grad_norm_)
    SKIP_NONFINITE_STEPS = False  # skip an update whose gradient norm is inf / NaN (weights, Adam state, EMA, step counts kept)
    EMA_DECAY = 0.0             # > 0: keep an exponential moving average of the weights (ema += (1 - decay)(w - ema) per update)
    EVAL_USE_EMA = False        # test_model / evaluate_seld / infer.py load the checkpoint's ema_state_dict (an error if absent)
    # SELD evaluation (seld_eval.py, trainer.evaluate_seld, infer.py)
    SELD_THRESHOLD = 0.5        # a grid cell is a detection when its meta-frame probability reaches this and beats its 8 neighbours
    SELD_MAX_PEAKS = 4          # detections kept per (100 ms meta-frame, class), 1..8
    SELD_DOA_THRESHOLD_DEG = 20  # a detection matches a reference within this great-circle angle (F20 / ER20)
    SELD_TTA_PATTERNS = ()      # test-time augmentation in evaluate_seld / infer.py: the spatial patterns (0..15, section 11.1)
                                # whose un-permuted grid maps are averaged before the peak test; () = off, "all" = the
                                # 16, or a list such as (0, 2, 9).  One forward per pattern; 4-channel FOA features only
    # Track linking of the decoded detections (seld_eval.track, csrc/seld_track.hip)
    SELD_TRACK = False          # evaluate_seld / infer.py link the frame-wise detections into tracks: the CSV's third column is
                                # then a track id, short tracks are dropped, short gaps filled
    SELD_TRACK_GATE_DEG = 20    # a detection continues a track when it lies within this great-circle angle of its last cell
    SELD_TRACK_MAX_GAP = 2      # a track survives this many meta-frames without a detection (they are filled), 0..16
    SELD_TRACK_MIN_LEN = 3      # tracks spanning fewer meta-frames (onset to offset) are removed
    # Sub-cell DOA refinement of the decoded detections (seld_eval.grid_decode_refine, csrc/seld_refine.hip)
    SELD_REFINE = False         # evaluate_seld / infer.py score and write a direction finer than the 10-degree cell: the
                                # probability-weighted mean of the unit vectors of the peak cell and its neighbours
    # Threshold sweep and per-class thresholds (seld_eval.sweep / apply_thresholds, csrc/seld_sweep.hip)
    SELD_SWEEP_THRESHOLDS = ()  # evaluate_seld also scores these detection thresholds from its one decode (at the lowest of
                                # them): a list, or a spelling such as "0.05:0.95:0.05" (start:stop:step); () = off.  Up to 64
    SELD_CLASS_THRESHOLDS = None  # 13 detection thresholds, one per class, or the path of a thresholds.json that a sweep
                                # wrote (thresholds_out); takes the place of SELD_THRESHOLD.  None = one threshold for all
    SELD_THRESHOLDS_OUT = None  # evaluate_seld writes the swept grid and its best global / per-class thresholds to this file
    # Segment-based, class-macro metrics (seld_eval.segment_metrics, csrc/seld_segment.hip)
    SELD_SEGMENT_METRICS = False  # evaluate_seld also reports F / ER / LE / LR and the SELD score per 1 s block and class,
                                # micro- and macro-averaged: the figures published SELD results are given in
    SELD_JACKKNIFE = False      # with SELD_SEGMENT_METRICS: 95 % confidence intervals from a jackknife over the recordings
    # Sample-rate conversion of the input (seld_native.resample, csrc/resample.hip)
    RESAMPLE_INPUT = False      # SELDDataset / audio_to_mel_spectrogram / infer.py convert recordings whose rate is not SR (48 kHz,
                                # 44.1 kHz, ...) to SR on the GPU before the feature kernels; off: such a recording raises

    def __init__(self):
        for folder in (self.OUTPUT_PATH, self.CHECKPOINT_PATH):
            folder.mkdir(exist_ok=True, parents=True)
        audio, meta = self.AUDIO_PATH, self.METADATA_PATH
        self.TRAIN_AUDIO_PATH = audio / "dev-train-sony" / self.TRAIN_AUDIO_FILE
        self.TRAIN_META_PATH = meta / "dev-train-sony" / self.TRAIN_META_FILE
        self.TEST_AUDIO_PATH = audio / "dev-test-sony" / self.TEST_AUDIO_FILE
        self.TEST_META_PATH = meta / "dev-test-sony" / self.TEST_META_FILE
        for site in ("SONY", "TAU"):
            for split in ("TRAIN", "TEST"):
                sub = f"dev-{split.lower()}-{site.lower()}"
                setattr(self, f"{site}_{split}_DIR", audio / sub)
                setattr(self, f"{site}_{split}_META_DIR", meta / sub)
