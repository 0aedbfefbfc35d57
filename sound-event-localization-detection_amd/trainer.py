"""Training / evaluation loops for SELD on MI355X (drop-in for the reference's ``trainer.py``).

``train_model`` / ``test_model`` keep the reference's signatures, return values, checkpoint format
and epoch semantics (trainer.py:23-392, :394-711):
  Adam(lr, weight_decay as L2-in-grad) + ReduceLROnPlateau(min, factor, patience) on the TEST loss,
  early stopping on the TRAIN loss (PATIENCE, MIN_DELTA), best checkpoint on the TEST loss,
  periodic checkpoints (keep last N), history dict, loss-curve PNG, reload of the best weights.

What is different underneath:
  * one process per GPU: under ``torchrun`` the model is wrapped in DistributedDataParallel
    (RCCL over xGMI, bucketed all-reduce overlapped with backward); window indices -- not files --
    are sharded across ranks so the window set is exactly the single-process one; the per-epoch
    loss sums are all-reduced so LR-plateau / early-stop / best-checkpoint decisions agree on
    every rank; rank 0 alone writes checkpoints, history and plots;
  * bf16 autocast + channels-last convolutions on ROCm devices (conv / linear / attention
    contractions on the matrix cores);
  * device feed: when the loader wraps our ``SELDDataset`` the batches are gathered on the GPU
    from the device-resident feature timeline and the compact uint16 label mask
    (seld_window_gather), so the 290 MB/step dense-label upload and the worker pipes disappear;
    the sampler's order (shuffle / sequential), batch size and drop_last are honoured;
  * fused softmax+MSE loss kernel; no per-step ``.item()`` host syncs (losses accumulate on
    the device and are read once per epoch).
"""
import gc
import logging
import math
import os
import random
from contextlib import nullcontext
from datetime import datetime
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader, RandomSampler, SequentialSampler  # noqa: F401
from tqdm import tqdm

import seld_augment
import seld_balance
import seld_standardise
from config import Config
from dataset import SELDDataset
from loss import SMRSELDLoss
from model import SMRSELDWithCSPDarkNet
from model_conformer import SELD_Conformer
from model_crnn import SELD_CRNN
from resnet50_model import SELD_ResNet50_Conformer
from seld_rnn import SeldGRU
from utils import get_local_rank, get_rank, get_world_size, safe_torch_load
from visualization import plot_loss_curves, visualize_grid_predictions, visualize_loss_components  # noqa: F401

logger = logging.getLogger("SMR_SELD")
config = Config()


# ------------------------------------------------------------------------------------------------
# model factory (trainer.py:50-95 / :432-473)
# ------------------------------------------------------------------------------------------------

def build_model(grid_size, use_small_model=True, model_type=None, n_channels=None):
    kind = config.MODEL_TYPE if model_type is None else model_type
    common = dict(n_channels=config.N_CHANNELS if n_channels is None else n_channels, grid_size=grid_size,
                  num_classes=config.NUM_CLASSES)
    if kind == "crnn":
        logger.info("Initializing CRNN model...")
        return SELD_CRNN(n_mels=config.N_MELS, cnn_channels=config.CRNN_CNN_CHANNELS,
                         rnn_hidden=config.CRNN_RNN_HIDDEN, rnn_layers=config.CRNN_RNN_LAYERS,
                         dropout=config.CRNN_DROPOUT, **common)
    if kind == "conformer":
        logger.info("Initializing Conformer model...")
        return SELD_Conformer(n_mels=config.N_MELS, cnn_channels=config.CRNN_CNN_CHANNELS,
                              conf_d_model=config.CONF_D_MODEL, conf_n_heads=config.CONF_N_HEADS,
                              conf_n_layers=config.CONF_N_LAYERS, conf_kernel_size=config.CONF_KERNEL_SIZE,
                              dropout=config.CONF_DROPOUT, **common)
    if kind == "resnet_conformer":
        logger.info("Initializing ResNet50-Conformer model...")
        return SELD_ResNet50_Conformer(n_mels=config.N_MELS, conf_d_model=config.RESNET_CONF_D_MODEL,
                                       conf_n_heads=config.RESNET_CONF_N_HEADS,
                                       conf_n_layers=config.RESNET_CONF_N_LAYERS,
                                       dropout=config.RESNET_DROPOUT, **common)
    logger.info("Initializing CSPDarkNet (CNN) model...")
    return SMRSELDWithCSPDarkNet(use_small=use_small_model, **common)


def prepare_model_for_device(model, device):
    """Move to the device; on a GPU use channels-last weights for the convolutions."""
    model = model.to(device)
    if device.type == "cuda" and getattr(config, "CHANNELS_LAST", True):
        model = model.to(memory_format=torch.channels_last)
    SeldGRU.fused_enabled = bool(getattr(config, "FUSED_GRU", True))
    if device.type == "cuda":
        import seld_convtail
        import seld_gru
        seld_convtail.enabled = bool(getattr(config, "FUSED_CONV_TAIL", True))
        import model_crnn
        model_crnn._Conv3x3.enabled = bool(getattr(config, "CONV_DGRAD_AS_FORWARD", True)) and \
            os.environ.get("SELD_CONV_AS_FWD", "1") != "0"          # developer switch for A/B runs
        model_crnn._Conv3x3.fused_wgrad = bool(getattr(config, "FUSED_CONV_WGRAD", True)) and \
            os.environ.get("SELD_CONV_WGRAD", "1") != "0"           # developer switch for A/B runs
        model_crnn._Conv3x3.fused_dgrad = bool(getattr(config, "FUSED_CONV_DGRAD", True)) and \
            os.environ.get("SELD_CONV_DGRAD", "1") != "0"           # developer switch for A/B runs
        model_crnn.ConvBlock.fused_fwd = bool(getattr(config, "FUSED_CONV_FWD", True)) and \
            os.environ.get("SELD_CONV_FWD", "1") != "0"             # developer switch for A/B runs
        import seld_convfirst
        seld_convfirst.enabled = bool(getattr(config, "FUSED_FIRST_BLOCK", True)) and \
            os.environ.get("SELD_FIRST_BLOCK", "1") != "0"          # developer switch for A/B runs
        if os.environ.get("SELD_DWCONV") is None:
            import seld_dwconv
            seld_dwconv.enabled = getattr(config, "FUSED_DWCONV", "auto")
            # "auto" weighed fewer GPU microseconds against more host work (round 1: +3 % at d_model 512, -7 % on the
            # host-bound d_model-256 Conformer); a captured iteration has no host work to weigh
            if seld_dwconv.enabled == "auto" and graph_step_enabled(device):
                seld_dwconv.enabled = True
        import seld_layernorm
        seld_layernorm.enabled = bool(getattr(config, "FUSED_LAYERNORM", True)) and \
            os.environ.get("SELD_LAYERNORM", "1") != "0"            # developer switch for A/B runs
        if os.environ.get("SELD_OVERLAP") is None:
            import seld_overlap
            seld_overlap.enabled = bool(getattr(config, "OVERLAP_WEIGHT_GRADS", True))
        import seld_linear
        seld_linear.conv1x1_as_gemm = bool(getattr(config, "CONV1X1_AS_GEMM", True)) and \
            os.environ.get("SELD_CONV1X1_GEMM", "1") != "0"         # developer switch for A/B runs
        import model_conformer
        model_conformer.MultiHeadSelfAttention.fused_qkv = bool(getattr(config, "FUSED_QKV", True)) and \
            os.environ.get("SELD_FUSED_QKV", "1") != "0"            # developer switch for A/B runs
        for module in model.modules():
            if isinstance(module, SeldGRU) and SeldGRU.fused_enabled:
                seld_gru.pack_parameters(module)
            if isinstance(module, model_conformer.MultiHeadSelfAttention):
                module.pack_parameters()
        if os.environ.get("SELD_CUT_LEVELS") is None:
            import seld_cut
            seld_cut.levels = int(getattr(config, "ALLREDUCE_CUT_LEVELS", 2))
        import seld_tuned
        seld_tuned.enable(device, bool(getattr(config, "TUNED_GEMMS", True)))
    SMRSELDLoss.fused_enabled = bool(getattr(config, "FUSED_LOSS", True))
    return model


def autocast_context(device):
    if device.type == "cuda" and getattr(config, "AMP_DTYPE", "bf16") == "bf16":
        return torch.autocast(device_type="cuda", dtype=torch.bfloat16)
    return nullcontext()


# ------------------------------------------------------------------------------------------------
# distributed plumbing
# ------------------------------------------------------------------------------------------------

def ensure_process_group(device):
    """Initialise torch.distributed when launched by torchrun (WORLD_SIZE > 1).  RCCL ('nccl') on
    GPUs, gloo on CPUs.  Returns (rank, world_size)."""
    world = get_world_size()
    if world <= 1:
        return 0, 1
    if not dist.is_initialized():
        # SELD_DIST_BACKEND=gloo on a GPU: the rehearsal mode in which several ranks share one device (RCCL refuses
        # that); gradients then travel through the host -- functional checks only
        backend = os.environ.get("SELD_DIST_BACKEND") or ("nccl" if device.type == "cuda" else "gloo")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if device.type == "cuda" and backend == "nccl":
            torch.cuda.set_device(device)
            dist.init_process_group(backend=backend, device_id=device)
        else:
            dist.init_process_group(backend=backend)
    return dist.get_rank(), dist.get_world_size()


def wrap_ddp(model, device, world):
    if world <= 1:
        return model
    if getattr(config, "SYNC_BATCHNORM", False) and device.type == "cuda":
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
    kwargs = dict(bucket_cap_mb=getattr(config, "DDP_BUCKET_MB", 25), gradient_as_bucket_view=True,
                  broadcast_buffers=False)
    if device.type == "cuda":
        kwargs.update(device_ids=[device.index], output_device=device.index)
    ddp = torch.nn.parallel.DistributedDataParallel(model, **kwargs)
    # DDP has just broadcast rank 0's parameters -- the bf16 working copies included.  The fp32 masters behind them
    # are not module parameters: broadcast them too (the reference never seeds, so every rank initialised its own)
    # and re-derive the working copies, or the ranks would part ways at the first optimiser step.
    _broadcast_masters(model)
    return ddp


def _broadcast_masters(model):
    state = getattr(model, "_seld_master_weights", None)
    if state is not None:
        with torch.no_grad():
            for master in state[1]:
                dist.broadcast(master, src=0)
            for p, master in zip(state[0], state[1]):
                p.data.copy_(master)


def broadcast_replica_state(model, world):
    """What constructing DistributedDataParallel does to the replicas, for the captured-step path that drives the
    gradient exchange itself (seld_graph.py): every rank takes rank 0's parameters, buffers and fp32 masters."""
    if world <= 1:
        return model
    with torch.no_grad():
        for t in list(model.parameters()) + list(model.buffers()):
            dist.broadcast(t.data, src=0)
    _broadcast_masters(model)
    return model


def all_reduce_sums(values, device):
    """Sum a small list of Python floats over all ranks (one collective per epoch phase)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return list(values)
    t = torch.tensor(values, dtype=torch.float64, device=device if device.type == "cuda" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.tolist()


def shard_indices(order, rank, world, pad=True):
    """DistributedSampler semantics on an explicit index order: pad (by wrapping) to a multiple of the
    world size so every rank runs the same number of steps, then take every world-th index."""
    order = list(order)
    if world <= 1:
        return order
    if pad and len(order) % world:
        order += order[: world - len(order) % world]
    return order[rank::world]


# ------------------------------------------------------------------------------------------------
# batch sources
# ------------------------------------------------------------------------------------------------

def epoch_order(n, shuffle, seed, epoch):
    """The index order of one epoch: a seeded permutation (the same on every rank) or sequential."""
    if shuffle:
        g = torch.Generator().manual_seed(seed * 100003 + epoch)
        return torch.randperm(n, generator=g).tolist()
    return list(range(n))


def batched(order, batch_size, drop_last):
    out = [order[lo:lo + batch_size] for lo in range(0, len(order), batch_size)]
    return out[:-1] if drop_last and out and len(out[-1]) < batch_size else out


class LoaderFeed:
    """The stock path: iterate the DataLoader the caller built (CPU tensors -> device).  With more than one rank the
    caller's loader would hand EVERY rank the full epoch (the reference is single-process: main.py:60-74 builds a plain
    shuffling DataLoader), so the epoch's index order is sharded like DeviceFeed's and a loader with the caller's
    batch size, workers, collate function and pinning is driven by an explicit batch sampler."""

    def __init__(self, loader, device, rank=0, world=1, seed=0):
        if seld_augment.enabled(config):
            # the augmentation lives in the device gather kernels (csrc/augment.hip); the product path has no CPU fallback
            on = [name for name in seld_augment.SWITCHES if getattr(config, name, 0)]
            raise RuntimeError(f"{', '.join(on)}: training augmentation is applied by the device window gather and needs the "
                               f"device feed (DEVICE_FEED = True, a ROCm GPU, a SELDDataset kept on the device); the host "
                               f"DataLoader path has no CPU implementation of it.  Switch the augmentation off to use it")
        if getattr(config, "STANDARDISE_FEATURES", False):
            # likewise: the statistics are reduced and applied by device kernels (csrc/standardise.hip, the affine gathers)
            raise RuntimeError("STANDARDISE_FEATURES: the per-bin standardisation is applied by the device window gather and "
                               "needs the device feed (DEVICE_FEED = True, a ROCm GPU, a SELDDataset kept on the device); the "
                               "host DataLoader path has no CPU implementation of it.  Switch it off to use this path")
        if getattr(config, "BALANCED_SAMPLING", False):
            # likewise: the per-window class statistics are reduced from the device-resident label mask (csrc/balance.hip)
            raise RuntimeError("BALANCED_SAMPLING: the windows' class statistics are reduced from the device-resident label mask "
                               "and need the device feed (DEVICE_FEED = True, a ROCm GPU, a SELDDataset kept on the device); "
                               "the host DataLoader path has no CPU implementation of it.  Switch it off to use this path")
        if getattr(config, "PCEN", False):
            # likewise: the recurrence along time is a device kernel (csrc/pcen.hip)
            raise RuntimeError("PCEN: the per-channel energy normalisation runs on the device-resident features and needs the "
                               "device feed (DEVICE_FEED = True, a ROCm GPU, a SELDDataset kept on the device); the host "
                               "DataLoader path has no CPU implementation of it.  Switch it off to use this path")
        self.loader, self.device = loader, device
        self.rank, self.world, self.seed = rank, world, seed
        sampler = getattr(loader, "sampler", None)
        self.shuffle = isinstance(sampler, RandomSampler)
        if world > 1 and getattr(loader, "batch_size", None) is None:
            raise ValueError("data-parallel training needs a DataLoader with a batch_size (got a batch_sampler-only loader)")
        if world > 1 and not isinstance(sampler, (RandomSampler, SequentialSampler)):
            # a Weighted / SubsetRandom / custom sampler cannot be sharded by re-deriving its order: refuse instead of
            # silently training on a different (sequential) order
            raise ValueError(f"data-parallel training shards the epoch's index order itself and supports the stock "
                             f"Random / Sequential samplers only (got {type(sampler).__name__})")
        if world > 1:
            n = len(loader.dataset)
            if n % world:
                logger.info(f"  data parallel: {world - n % world} window(s) of every epoch are seen twice (the index "
                            f"order is padded by wrapping to a multiple of {world} ranks, DistributedSampler semantics)")

    def _batches_of_rank(self, epoch):
        order = shard_indices(epoch_order(len(self.loader.dataset), self.shuffle, self.seed, epoch), self.rank, self.world)
        return batched(order, self.loader.batch_size, bool(self.loader.drop_last))

    def __len__(self):
        return len(self.loader) if self.world <= 1 else len(self._batches_of_rank(0))

    def batches(self, epoch):
        loader = self.loader
        if self.world > 1:
            # the caller's loader with this rank's batches: workers, collate function, pinning, worker initialisation,
            # generator and prefetch depth are carried over
            extra = {}
            if loader.num_workers > 0:
                extra = dict(prefetch_factor=loader.prefetch_factor, worker_init_fn=loader.worker_init_fn,
                             multiprocessing_context=loader.multiprocessing_context)
            loader = DataLoader(loader.dataset, batch_sampler=self._batches_of_rank(epoch), num_workers=loader.num_workers,
                                collate_fn=loader.collate_fn, pin_memory=loader.pin_memory, generator=loader.generator,
                                timeout=loader.timeout, **extra)
        for spectrograms, labels in loader:
            yield (spectrograms.to(self.device, non_blocking=True), labels.to(self.device, non_blocking=True))


class DeviceFeed:
    """Batches gathered on the GPU from the dataset's device timeline.  Honours the DataLoader's
    batch size, drop_last and sampler kind (RandomSampler -> a fresh permutation every epoch,
    otherwise sequential); shards the index order over the ranks.  With Config.BALANCED_SAMPLING a shuffling loader's
    epochs are class-balanced draws with replacement instead (seld_balance.py) -- for the caller
    that asks for them, which is the training loop."""

    def __init__(self, loader, device, rank, world, seed=0):
        self.dataset = loader.dataset
        self.batch_size = loader.batch_size
        self.drop_last = bool(loader.drop_last)
        self.shuffle = isinstance(loader.sampler, RandomSampler)
        self.device, self.rank, self.world, self.seed = device, rank, world, seed
        # a spatial swap the feature set does not define is refused when the feed is built, not at the first batch
        # the array is the DATASET's (Config.MIC_POSITIONS as of its construction: what its gathers work with)
        self.array = getattr(self.dataset, "mic_array", None)
        if seld_augment.enabled(config):
            # a Config that says otherwise by now would have the draw and the gathers disagree
            now = seld_augment.mic_positions(getattr(config, "MIC_POSITIONS", None))
            if (self.array is None) != (now is None) or (now is not None and not np.array_equal(self.array, now)):
                raise ValueError("Config.MIC_POSITIONS differs from the positions this dataset was constructed with "
                                 "(SELDDataset.mic_array): construct the dataset under the setting the training runs with")
            # (a dataset whose timeline holds PCEN values refuses the switches defined on dB or power values, whatever
            # Config.PCEN says by now)
            seld_augment.check_settings(config, getattr(config, "FEATURE_SET", "logmel"), self.dataset.n_channels,
                                        array=self.array,
                                        pcen=bool(getattr(config, "PCEN", False))
                                        or getattr(self.dataset, "pcen_settings", None) is not None)
            if seld_augment.settings(config)["rotate"] and getattr(self.dataset, "rot_tm", None) is None:
                raise ValueError("AUGMENT_ROTATE needs a dataset constructed with the switch on and kept on the device: the "
                                 "rotating gather reads three extra mel rows per frame of the timeline (SELDDataset.rot_tm)")
            if seld_augment.settings(config)["mix_prob"] > 0 and getattr(self.dataset, "rot_tm", None) is not None:
                raise ValueError("AUGMENT_MIX_PROB cannot be used with a dataset constructed with AUGMENT_ROTATE: its batches "
                                 "come from the rotating gathers, which do not mix (construct the dataset with the switch off)")
        # Config.BALANCED_SAMPLING: out-of-range settings are refused here; the weight table is built on first use
        self.balanced = bool(getattr(config, "BALANCED_SAMPLING", False)) and self.shuffle
        self._balance_settings = seld_balance.check_settings(config) if getattr(config, "BALANCED_SAMPLING", False) else None
        self._balance_k = None

    def balance_table(self):
        """The int64 weight table ``k`` of class-balanced sampling (seld_balance.window_weights of the dataset's
        window_class_counts), built once.  Every rank reduces its own copy of the label timeline; under data parallelism
        rank 0's CRC32 of the table travels the way make_feed's seed does, and a rank whose table differs raises here --
        before the first batch -- instead of training on overlapping shards."""
        if self._balance_k is None:
            if self._balance_settings is None:
                raise RuntimeError("balance_table: Config.BALANCED_SAMPLING was off when this feed was built")
            k, failure = None, None
            try:
                k = seld_balance.window_weights(self.dataset.window_class_counts(), self._balance_settings)
            except ValueError as exc:                    # (no active window): raised BEHIND the collectives below, so that
                if self.world <= 1:                      # a rank that fails alone leaves no other rank waiting in them
                    raise
                failure = exc
            if self.world > 1:
                mine = seld_balance.table_crc(k) if failure is None else 1 << 32          # no CRC32: agrees with no table
                first = int(all_reduce_sums([float(mine) if self.rank == 0 else 0.0], self.device)[0])
                agree = all_reduce_sums([1.0 if mine == first and failure is None else 0.0], self.device)[0]
                if failure is not None:
                    raise failure
                if int(agree) != self.world:             # every rank raises, none is left waiting in a collective
                    raise RuntimeError(f"BALANCED_SAMPLING: rank {self.rank}'s weight table (CRC32 {mine:08x}) "
                                       f"{'differs from' if mine != first else 'is'} rank 0's ({first:08x}), and "
                                       f"{self.world - int(agree)} rank(s) disagree: the ranks' datasets differ, their "
                                       f"epoch orders would overlap")
            self._balance_k = k
        return self._balance_k

    def _order(self, epoch, balanced=True):
        """This rank's window indices of ``epoch``.  ``balanced``: the caller takes the class-balanced draw when the feed
        has one (Config.BALANCED_SAMPLING on a shuffling loader); with the switch off it is ``epoch_order``'s, as ever.
        The defaults differ ON PURPOSE: ``_order(epoch)`` answers "what does the training loop see in this epoch" (the
        balanced order with the switch on), while ``batches`` hands the balanced order only to the caller that asks for it
        and passes its own flag down -- an evaluation loop over a shuffling loader gets the permutation.  A caller of
        ``_order`` that is not the training loop passes ``balanced=False``."""
        if balanced and self.balanced:
            order = seld_balance.order(self.balance_table(), self.seed, epoch).tolist()
            return shard_indices(order, self.rank, self.world)
        return shard_indices(epoch_order(len(self.dataset), self.shuffle, self.seed, epoch), self.rank, self.world)

    def __len__(self):
        n = len(shard_indices(range(len(self.dataset)), self.rank, self.world))
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def batches(self, epoch, out=None, augment=False, balanced=False):
        """``out``: see SELDDataset.device_batch (gather straight into a captured step's input buffers).
        ``augment``: apply the Config.AUGMENT_* switches (seld_augment.draw: a window's transform depends on the seed, the
        epoch and the window's dataset index only).  Only the training loop passes True; with every switch off it is the
        plain gather.
        ``balanced``: take the class-balanced order (Config.BALANCED_SAMPLING).  Only the training loop passes True; with
        the switch off it is the permutation.  A balanced epoch holds windows several times, so the augmentation streams
        are keyed on each draw's position in the epoch's GLOBAL order (rank + world * local position) instead of the
        window index: every copy of an oversampled window gets a transform of its own."""
        augment = bool(augment) and seld_augment.enabled(config)
        balanced = bool(balanced) and self.balanced
        # AUGMENT_MIX_PROB: a partner per window from a stream of its own (seld_augment.draw_mix; csrc/mix.hip)
        mixing = augment and seld_augment.settings(config)["mix_prob"] > 0
        # frequency shift, level / filter curve, cutouts: a third stream per window (seld_augment.draw_spectral), applied by
        # one in-place stage behind whichever gather produced the batch (csrc/spectral.hip)
        shaping = augment and seld_augment.spectral_enabled(config)
        done = 0                                             # windows of this rank's order already handed out
        for idx in batched(self._order(epoch, balanced), self.batch_size, self.drop_last):
            keys = [self.rank + self.world * (done + j) for j in range(len(idx))] if balanced else None
            done += len(idx)
            params = seld_augment.draw(self.seed, epoch, idx, config, window=self.dataset.window_length_frames,
                                       array=self.array, keys=keys) if augment else None
            more = {}
            if shaping:
                more["spectral"] = seld_augment.draw_spectral(self.seed, epoch, idx, config,
                                                              window=self.dataset.window_length_frames, keys=keys)
            if not mixing:
                yield self.dataset.device_batch(idx, out=out, augment=params, **more)
                continue
            mix = seld_augment.draw_mix(self.seed, epoch, idx, config, len(self.dataset), keys=keys)
            yield self.dataset.device_batch(idx, out=out, augment=params, mix=mix, **more)


def make_feed(loader, device, rank, world):
    ds = loader.dataset
    use_device = (getattr(config, "DEVICE_FEED", True) and device.type == "cuda" and isinstance(ds, SELDDataset)
                  and getattr(ds, "spec_tm", None) is not None and loader.batch_size is not None)
    seed = config.SEED if getattr(config, "SEED", None) is not None else random.randrange(1 << 30)
    if world > 1:                          # every rank must draw the same permutation
        seed = int(all_reduce_sums([float(seed) if rank == 0 else 0.0], device)[0])
    if use_device:
        return DeviceFeed(loader, device, rank, world, seed)
    return LoaderFeed(loader, device, rank, world, seed)


# ------------------------------------------------------------------------------------------------
# one optimisation step (shared with bench.py)
# ------------------------------------------------------------------------------------------------

def train_step(model, criterion, optimizer, spectrograms, labels, device):
    """forward (autocast) -> loss -> backward (DDP all-reduce overlaps here) -> Adam.  Returns the
    detached (total, class) loss tensors; nothing is synchronised with the host."""
    optimizer.zero_grad(set_to_none=True)
    with autocast_context(device):
        predictions = model(spectrograms)
    total, term = criterion.loss_tensor(predictions, labels)
    total.backward()
    optimizer.step()
    return total.detach(), term.detach()


def eval_step(model, criterion, spectrograms, labels, device):
    with autocast_context(device):
        predictions = model(spectrograms)
    total, term = criterion.loss_tensor(predictions, labels)
    return predictions, total.detach(), term.detach()


# ------------------------------------------------------------------------------------------------
# fp32 master weights behind bf16 working copies
# ------------------------------------------------------------------------------------------------
# Under autocast every conv / Linear / GRU weight is cast fp32 -> bf16 once per iteration and every weight gradient
# bf16 -> fp32: one tiny kernel each (36 per CRNN iteration, 336 per ResNet50-Conformer iteration, ~5 us apiece on an
# otherwise GPU-bound step).  With MASTER_WEIGHTS the model holds the bf16 values themselves -- bit-identical to what
# autocast would produce from the fp32 masters -- and the optimiser owns the fp32 masters: per iteration ONE
# multi-tensor copy of the bf16 gradients into the masters' fp32 gradients, fused Adam on the masters, ONE
# multi-tensor copy back.  Under DDP the weight gradients are then all-reduced in bf16 (half the xGMI bytes).
# BatchNorm / LayerNorm parameters and the GRU / convolution biases stay fp32 (autocast keeps those ops in fp32 as well);
# nn.Linear biases are working copies too (the GEMM epilogue adds them in the compute dtype either way).

def enable_master_weights(model, device):
    """Convert in place; returns True when active.  Call before wrap_ddp / make_optimizer."""
    if not (device.type == "cuda" and getattr(config, "MASTER_WEIGHTS", True)
            and getattr(config, "AMP_DTYPE", "bf16") == "bf16"):
        return False
    import seld_gru
    target = unwrap(model)
    low, masters, names = [], [], {}
    for mod_name, module in target.named_modules():
        if not isinstance(module, (torch.nn.Conv1d, torch.nn.Conv2d, torch.nn.Linear, torch.nn.GRU)):
            continue
        for pname, p in module.named_parameters(recurse=False):
            # weight matrices, and the biases of Linear layers (they enter the GEMM epilogue in the compute dtype: a
            # per-iteration cast otherwise); GRU / conv / norm biases stay fp32 (kernels that read them in fp32)
            working = p.ndim >= 2 or (isinstance(module, torch.nn.Linear) and pname == "bias")
            if working and p.dtype == torch.float32 and p.requires_grad:
                master = p.detach().clone()
                p.data = p.data.to(torch.bfloat16)
                low.append(p)
                masters.append(master)
                names[f"{mod_name}.{pname}" if mod_name else pname] = master
        if isinstance(module, SeldGRU) and SeldGRU.fused_enabled:
            seld_gru.pack_parameters(module)          # keep (forward, reverse) pairs adjacent in their new dtype
    for module in target.modules():                   # q / k / v of the attention layers likewise (seld_pack.py)
        if type(module).__name__ == "MultiHeadSelfAttention" and hasattr(module, "pack_parameters"):
            module.pack_parameters()
    target._seld_master_weights = (low, masters, names)
    return True


def disable_master_weights(model):
    """Give the model its fp32 weights back (what ``train_model`` returns and what checkpoints hold)."""
    target = unwrap(model)
    state = getattr(target, "_seld_master_weights", None)
    if state is None:
        return
    for p, master in zip(state[0], state[1]):
        p.data = master.detach().clone()
        p.grad = None
    del target._seld_master_weights


def model_state_dict(model):
    """``state_dict`` with the fp32 masters in place of the bf16 working copies (checkpoint format unchanged)."""
    target = unwrap(model)
    sd = target.state_dict()
    state = getattr(target, "_seld_master_weights", None)
    if state is not None:
        for name, master in state[2].items():
            sd[name] = master.detach().clone()
    return sd


class MasterWeightAdam(torch.optim.Adam):
    """Adam over (fp32 masters of the bf16 working weights) + (the remaining fp32 parameters)."""

    def __init__(self, low, masters, others, **kwargs):
        super().__init__(list(masters) + list(others), **kwargs)
        self._low, self._masters, self._others = list(low), list(masters), list(others)
        self.fused_casts = self.fallback_casts = 0        # how often the one-launch casts applied (diagnostics)
        self.own_steps = 0                                # updates done by csrc/adam.hip
        self._uniform_steps = True                        # every parameter has been updated in every step so far
        self._adam_cache = {}
        if os.environ.get("SELD_OWN_ADAM") == "0":
            self.own_kernel = False
        self._grad_cast_cache, self._weight_cast_cache = {}, {}
        for m in self._masters:
            m.grad = torch.zeros_like(m)

    own_kernel = True         # Config.FUSED_ADAM_KERNEL via make_optimizer; SELD_OWN_ADAM=0 switches it off (developer A/B)
    # the guarded update, all off: configure_guard() switches them on and makes the device tensors
    grad_clip_norm = 0.0      # Config.GRAD_CLIP_NORM
    skip_nonfinite = False    # Config.SKIP_NONFINITE_STEPS
    ema_decay = 0.0           # Config.EMA_DECAY
    _guard = _partial = _ema = None
    seld_grad_scale = 1.0          # every gradient is multiplied by this on its way into the update (data parallel: 1 / world,
                              # set by seld_graph.GraphedTrainStep -- folded into the kernel instead of a pass over the buffers)

    def configure_guard(self, grad_clip_norm=0.0, skip_nonfinite=False, ema_decay=0.0):
        """Switch on gradient-norm clipping / the non-finite step skip / the weight EMA.  Allocates what the device side
        needs ONCE, before any capture: the guard record, the norm's partial scratch and the EMA tensors (copies of the
        masters and of the fp32 others, kept outside ``self.state``: ``state_dict()`` keeps the framework's format)."""
        import seld_native
        grad_clip_norm, ema_decay = float(grad_clip_norm), float(ema_decay)
        if not (grad_clip_norm >= 0.0 and math.isfinite(grad_clip_norm)):
            raise ValueError(f"GRAD_CLIP_NORM must be a finite number >= 0, got {grad_clip_norm}")
        if not 0.0 <= ema_decay < 1.0:
            raise ValueError(f"EMA_DECAY must be in [0, 1), got {ema_decay}")
        self.grad_clip_norm, self.skip_nonfinite, self.ema_decay = grad_clip_norm, bool(skip_nonfinite), ema_decay
        params = self._masters + self._others
        if self._uses_norm and self._guard is None:
            device = params[0].device
            self._guard = seld_native.new_guard_record(device)
            self._partial = torch.zeros(seld_native.grad_norm_scratch_floats([p.numel() for p in params]),
                                        dtype=torch.float32, device=device)
        if ema_decay > 0.0 and self._ema is None:
            self._ema = [p.detach().clone(memory_format=torch.preserve_format) for p in params]
        if ema_decay == 0.0:
            self._ema = None
        self._norm_cache, self._guarded_cache = {}, {}
        return self

    @property
    def _uses_norm(self):
        return self.grad_clip_norm > 0.0 or self.skip_nonfinite

    @property
    def guard_active(self):
        return self._uses_norm or self.ema_decay > 0.0

    def guard_report(self):
        """{grad_norm, clip_coef, steps_skipped, steps_clipped} of the latest update / so far: one device-to-host copy
        (synchronises; call it per epoch, not per step)."""
        import seld_native
        if self._guard is None:
            return {"grad_norm": 0.0, "clip_coef": 1.0, "steps_skipped": 0, "steps_clipped": 0}
        rec = seld_native.read_guard(self._guard)
        return {k: rec[k] for k in ("grad_norm", "clip_coef", "steps_skipped", "steps_clipped")}

    def ema_tensors(self):
        """The EMA of every optimiser tensor, in the order masters + others (None when EMA_DECAY is 0)."""
        return self._ema

    def _torch_guard(self, grads):
        """The guard record from framework ops (the fallback's fallback: a gradient multi_grad_norm does not take)."""
        norms = torch._foreach_norm([g.float() for g in grads])
        total = (torch.linalg.vector_norm(torch.stack(norms).double()) * float(self.seld_grad_scale)).float()
        rec = self._guard
        coef = torch.clamp(self.grad_clip_norm / (total + 1e-6), max=1.0) if self.grad_clip_norm > 0.0 else torch.ones_like(total)
        apply = torch.isfinite(total).float() if self.skip_nonfinite else torch.ones_like(total)
        rec[0], rec[1], rec[2], rec[3] = total, coef, apply, 1.0 - apply
        counters = rec.view(torch.int32)
        counters[4] += (1.0 - apply).to(torch.int32)
        counters[5] += ((coef < 1.0) & (apply > 0)).to(torch.int32)

    def _own_step(self):
        """The whole update as ONE multi-tensor launch per 48 tensors (csrc/adam.hip): the bf16 gradients are read as they
        are and the bf16 working copies written from the new masters in the same pass -- 28 B per parameter instead of the
        40 B of cast + fused Adam + cast.  The framework's fused Adam formulas (agreement to rounding); the state keeps its format
        (per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq``), so ``state_dict`` is unchanged.  Returns False when the
        call does not qualify (then the three-launch path below runs)."""
        import seld_native
        group = self.param_groups[0]
        lr = group["lr"]
        if not (self.own_kernel and self._uniform_steps and len(self.param_groups) == 1 and isinstance(lr, torch.Tensor)
                and lr.is_cuda and not group.get("amsgrad") and not group.get("maximize")
                and not group.get("decoupled_weight_decay", False)):
            return False
        external = getattr(self, "external_master_grads", False)
        params = self._masters + self._others
        grads = [(m.grad if external else p.grad) for p, m in zip(self._low, self._masters)] + [p.grad for p in self._others]
        if any(g is None for g in grads):
            return False
        steps = []
        for p in params:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            steps.append(st["step"])
        lows = [p.data for p in self._low] + [None] * len(self._others)
        exp_avgs = [self.state[p]["exp_avg"] for p in params]
        exp_avg_sqs = [self.state[p]["exp_avg_sq"] for p in params]
        # descriptor checks first (nothing may have run when this returns False): a dry call with count 0 is not
        # available, so the eligibility test is multi_adam's own and the step counts are advanced only after it passed
        beta1, beta2 = group["betas"]
        if not self._adam_checked(grads, params, exp_avgs, exp_avg_sqs, lows):
            return False
        if self.guard_active:
            return self._own_guarded_step(group, grads, params, exp_avgs, exp_avg_sqs, lows, steps)
        torch._foreach_add_(steps, 1)                 # every parameter's own counter, as the framework keeps them
        ok = seld_native.multi_adam(grads, params, exp_avgs, exp_avg_sqs, lows, lr, steps[0], beta1, beta2, group["eps"],
                                    group["weight_decay"], float(self.seld_grad_scale), self._adam_cache)
        assert ok
        self.fused_casts += 1
        self.own_steps += 1
        return True

    def _own_guarded_step(self, group, grads, params, exp_avgs, exp_avg_sqs, lows, steps):
        """The update with a switch on: [norm of all gradients -> guard record] + the guarded one-launch Adam (clip
        coefficient, skip, EMA inside the same pass).  Device-side only: the step counts advance before the launch and
        are taken back by the record's ``skipped`` flag (0.0 or 1.0) after it, as torch's fused Adam does for found_inf."""
        import seld_native
        emas = self._ema
        if emas is not None and not all(e.dtype == torch.float32 and seld_native._dense_like(e, p)
                                        for e, p in zip(emas, params)):
            return False
        beta1, beta2 = group["betas"]
        scale = float(self.seld_grad_scale)
        torch._foreach_add_(steps, 1)
        guard = None
        if self._uses_norm:
            guard = self._guard
            ok = seld_native.multi_grad_norm(grads, guard, self._partial, scale, self.grad_clip_norm, self.skip_nonfinite,
                                             self._norm_cache)
            assert ok
        ok = seld_native.multi_adam_guarded(grads, params, exp_avgs, exp_avg_sqs, lows, group["lr"], steps[0], beta1, beta2,
                                            group["eps"], group["weight_decay"], scale, emas, self.ema_decay, guard,
                                            self._guarded_cache)
        assert ok
        if self.skip_nonfinite:
            torch._foreach_add_(steps, guard[3], alpha=-1)
        self.fused_casts += 1
        self.own_steps += 1
        return True

    def _adam_checked(self, grads, params, exp_avgs, exp_avg_sqs, lows):
        import seld_native
        for g, p, m, v, lo in zip(grads, params, exp_avgs, exp_avg_sqs, lows):
            if not (p.is_cuda and p.dtype == torch.float32 and g.dtype in (torch.float32, torch.bfloat16)
                    and seld_native._dense_like(g, p) and seld_native._dense_like(m, p) and seld_native._dense_like(v, p)
                    and (lo is None or (lo.dtype == torch.bfloat16 and seld_native._dense_like(lo, p)))):
                return False
        return True

    @torch.no_grad()
    def step(self, closure=None):
        import seld_native
        if self._own_step():
            return None
        grads = [p.grad for p in self._low]
        if any(p.grad is None for p in self._low + self._others):
            self._uniform_steps = False           # the framework skips such parameters: their step counts fall behind
        if self._uses_norm:
            # the norm of the gradients as stored, times grad_scale (before the in-place scaling below rounds them)
            external = getattr(self, "external_master_grads", False)
            raw = [(m.grad if external else p.grad) for p, m in zip(self._low, self._masters)] + [p.grad for p in self._others]
            if any(g is None for g in raw):
                raise RuntimeError("the guarded update needs a gradient for every parameter")
            if not seld_native.multi_grad_norm(raw, self._guard, self._partial, float(self.seld_grad_scale),
                                               self.grad_clip_norm, self.skip_nonfinite, self._norm_cache):
                self._torch_guard(raw)
        if self.seld_grad_scale != 1.0:
            external = getattr(self, "external_master_grads", False)
            scaled = [g for g in ([m.grad for m in self._masters] if external else grads) + [p.grad for p in self._others]
                      if g is not None]
            torch._foreach_mul_(scaled, float(self.seld_grad_scale))
        master_grads = [m.grad for m in self._masters]
        if getattr(self, "external_master_grads", False):
            # the data-parallel exchange reduced in fp32: the masters' gradients ARE the all-reduced flat buffer's views
            # (seld_graph.FlatGradients, wire dtype "fp32"), nothing to cast
            self.fused_casts += 1
        elif all(g is not None for g in grads) and seld_native.multi_cast(grads, master_grads, self._grad_cast_cache):
            self.fused_casts += 1
        else:
            self.fallback_casts += 1
            for m, g in zip(self._masters, grads):       # a parameter without a gradient, or a layout mismatch
                m.grad.zero_() if g is None else m.grad.copy_(g)
        if self.grad_clip_norm > 0.0:
            torch._foreach_mul_([m.grad for m in self._masters] + [p.grad for p in self._others], self._guard[1])
        if self.skip_nonfinite:
            self.found_inf = self._guard[3]          # torch's fused Adam: no update and the step counts taken back, on the device
        try:
            out = super().step(closure)
        finally:
            if self.skip_nonfinite:
                del self.found_inf
        if self._ema is not None:
            params = self._masters + [p.data for p in self._others]
            if self._uses_norm:
                weight = self._guard[2] * (1.0 - self.ema_decay)          # 0 on a skipped step
                torch._foreach_lerp_(self._ema, params, [weight] * len(params))
            else:
                torch._foreach_lerp_(self._ema, params, 1.0 - self.ema_decay)
        working = [p.data for p in self._low]
        if not seld_native.multi_cast(self._masters, working, self._weight_cast_cache):
            torch._foreach_copy_(working, self._masters)
        return out

    def zero_grad(self, set_to_none=True):
        for p in self._low + self._others:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()


def graph_step_enabled(device, world=1):
    """Captured training iterations (seld_graph.py): ROCm device, Config.GRAPH_STEP, and no SyncBatchNorm (its
    collectives sit inside the forward pass, which the captured path never interrupts)."""
    return (device.type == "cuda" and bool(getattr(config, "GRAPH_STEP", True))
            and os.environ.get("SELD_GRAPH_STEP", "1") != "0"
            and not (world > 1 and getattr(config, "SYNC_BATCHNORM", False)))


def make_optimizer(model, learning_rate, device, capturable=False):
    kwargs = dict(lr=learning_rate, weight_decay=config.WEIGHT_DECAY)
    if device.type == "cuda":
        kwargs["fused"] = True            # one multi-tensor kernel instead of ~4 launches per parameter
        if capturable:                    # step count and learning rate live on the device (graph replay)
            kwargs["capturable"] = True
            kwargs["lr"] = torch.tensor(float(learning_rate), dtype=torch.float32, device=device)
    state = getattr(unwrap(model), "_seld_master_weights", None)
    clip, skip, decay = guard_settings()
    if state is not None:
        low_ids = {id(p) for p in state[0]}
        others = [p for p in model.parameters() if id(p) not in low_ids]
        opt = MasterWeightAdam(state[0], state[1], others, **kwargs)
        if not getattr(config, "FUSED_ADAM_KERNEL", True):
            opt.own_kernel = False
        if clip > 0.0 or skip or decay > 0.0:
            opt.configure_guard(clip, skip, decay)
        return opt
    if clip > 0.0 or skip or decay > 0.0:
        raise ValueError("GRAD_CLIP_NORM / SKIP_NONFINITE_STEPS / EMA_DECAY run inside the master-weight update on a ROCm "
                         "device (AMP_DTYPE = 'bf16', MASTER_WEIGHTS = True): there is no CPU or fp32 fallback")
    return torch.optim.Adam(model.parameters(), **kwargs)


def guard_settings():
    """(GRAD_CLIP_NORM, SKIP_NONFINITE_STEPS, EMA_DECAY) of the config, validated."""
    clip = float(getattr(config, "GRAD_CLIP_NORM", 0.0) or 0.0)
    skip = bool(getattr(config, "SKIP_NONFINITE_STEPS", False))
    decay = float(getattr(config, "EMA_DECAY", 0.0) or 0.0)
    if not (clip >= 0.0 and math.isfinite(clip)):
        raise ValueError(f"GRAD_CLIP_NORM must be a finite number >= 0, got {clip}")
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"EMA_DECAY must be in [0, 1), got {decay}")
    return clip, skip, decay


def ema_state_dict(model, optimizer):
    """``model_state_dict`` with every parameter replaced by its exponential moving average (fp32, the reference's keys);
    buffers (BatchNorm running statistics, ...) are the live model's.  None when the optimiser keeps no EMA."""
    emas = optimizer.ema_tensors() if hasattr(optimizer, "ema_tensors") else None
    if emas is None:
        return None
    ema_of = {id(p): e for p, e in zip(optimizer._low + optimizer._others, emas)}
    sd = model_state_dict(model)
    for name, p in unwrap(model).named_parameters():
        if id(p) in ema_of:
            sd[name] = ema_of[id(p)].detach().clone()
    return sd


def select_state_dict(checkpoint, use_ema=None):
    """The weights evaluation loads from a checkpoint: ``ema_state_dict`` when ``use_ema`` (default: Config.EVAL_USE_EMA)
    -- an error when the checkpoint has none, never a silent fallback -- else ``model_state_dict``."""
    if use_ema is None:
        use_ema = bool(getattr(config, "EVAL_USE_EMA", False))
    if not use_ema:
        return checkpoint["model_state_dict"]
    if checkpoint.get("ema_state_dict") is None:
        raise KeyError("EVAL_USE_EMA / use_ema is set but the checkpoint holds no 'ema_state_dict' (train with EMA_DECAY > 0)")
    return checkpoint["ema_state_dict"]


def make_stepper(model, criterion, optimizer, device, world=1):
    """The per-iteration callable of the epoch loop: ``(spectrograms, labels) -> (total, term)``.  On a ROCm device a
    ``seld_graph.GraphedTrainStep`` (captured iteration, flat-buffer gradient exchange); otherwise ``train_step``."""
    if graph_step_enabled(device, world) and not isinstance(model, torch.nn.parallel.DistributedDataParallel):
        import seld_graph
        return seld_graph.GraphedTrainStep(model, criterion, optimizer, device, world,
                                           autocast=lambda: autocast_context(device),
                                           overlap_allreduce=bool(getattr(config, "OVERLAP_ALLREDUCE", True)),
                                           reduce_dtype=getattr(config, "GRAD_REDUCE_DTYPE", "param"))
    return lambda spectrograms, labels: train_step(model, criterion, optimizer, spectrograms, labels, device)


def standardise_datasets(train_dataset, test_dataset):
    """Config.STANDARDISE_FEATURES: the statistics of the TRAINING dataset's timeline, set on both
    datasets (the test windows are standardised with the training statistics, never their own).  Returns the payload the
    checkpoints carry under ``feature_statistics``; None -- and nothing is computed, launched or set -- with the switch off."""
    if not getattr(config, "STANDARDISE_FEATURES", False):
        for ds in (train_dataset, test_dataset):           # statistics an earlier run with the switch on left behind
            if getattr(ds, "feature_stats", None) is not None:
                ds.set_feature_statistics(None)
        return None
    for ds in (train_dataset, test_dataset):
        if not isinstance(ds, SELDDataset) or getattr(ds, "spec_tm", None) is None:
            raise RuntimeError("STANDARDISE_FEATURES needs SELDDatasets that keep their device timeline (DEVICE_FEED = True, "
                               "keep_on_device=True): there is no CPU fallback")
    stats = train_dataset.feature_statistics()
    train_dataset.set_feature_statistics(stats)
    test_dataset.set_feature_statistics(stats)
    flat = int((stats["std"] < seld_standardise.FLAT_STD).sum())
    logger.info(f"Feature standardisation: {stats['frames']} training frames, {train_dataset.n_channels} x 64 bins"
                + (f", {flat} flat bin(s) only centred" if flat else ""))
    return seld_standardise.to_payload(stats, getattr(config, "FEATURE_SET", "logmel"), train_dataset.n_channels)


def log_balanced_sampling(train_feed):
    """Config.BALANCED_SAMPLING: build the training feed's weight table now -- the ranks compare
    theirs here, before the first batch -- and log once what it does to the classes' and the silent windows' exposure.
    Nothing is computed or launched with the switch off.  Returns the exposure report, or None."""
    if not getattr(config, "BALANCED_SAMPLING", False):
        return None
    if not isinstance(train_feed, DeviceFeed):
        raise RuntimeError("BALANCED_SAMPLING needs the device feed (DEVICE_FEED = True, a ROCm GPU, a SELDDataset kept on "
                           "the device): there is no CPU fallback")
    if not train_feed.balanced:
        logger.info("Balanced sampling: the training loader does not shuffle; its sequential order is kept")
        return None
    report = seld_balance.exposure(train_feed.dataset.window_class_counts(), train_feed.balance_table(),
                                   train_feed._balance_settings)
    logger.info("Balanced sampling: " + seld_balance.describe(report, train_feed.dataset.num_classes))
    return report


def apply_checkpoint_statistics(checkpoint, dataset):
    """Evaluation: the checkpoint decides.  Its ``feature_statistics`` are set on ``dataset`` when it holds them; without
    them the dataset gathers raw features -- unless Config.STANDARDISE_FEATURES is on, which is an error (the shape of the
    EVAL_USE_EMA one: never a silent evaluation on other inputs than the weights were trained on).  Returns the statistics."""
    stats = seld_standardise.checkpoint_statistics(checkpoint, config, channels=getattr(dataset, "n_channels", None))
    if hasattr(dataset, "set_feature_statistics"):
        if stats is not None or getattr(dataset, "feature_stats", None) is not None:
            dataset.set_feature_statistics(stats)
    elif stats is not None:
        raise RuntimeError("the checkpoint holds feature_statistics: evaluation needs an SELDDataset, whose device gathers "
                           "apply them")
    return stats


NIPD_SETTINGS = ("NIPD_MIN_HZ", "NIPD_MAX_HZ", "SOUND_SPEED")
PCEN_SETTINGS = seld_augment.PCEN_SETTINGS     # Config.PCEN and its five settings


def checkpoint_pcen_settings(checkpoint):
    """The PCEN settings a checkpoint's config records (``checkpoint_payload`` pins them with the switch on), in the form
    of ``SELDDataset.pcen_settings``; None when it records none or the switch off."""
    own = getattr(checkpoint.get("config"), "__dict__", {})
    if not own.get("PCEN", False):
        return None
    return {name: float(own.get(name, getattr(Config, name))) for name in PCEN_SETTINGS[1:]}


def check_dataset_pcen(expected, dataset, who):
    """Raise ValueError when ``dataset`` was built with other PCEN settings than ``expected`` (``who`` says whose they
    are): the weights would see other input values than they were trained on."""
    built = getattr(dataset, "pcen_settings", None)
    if built != expected:
        say = lambda p: "PCEN off" if p is None else "PCEN on with " + ", ".join(f"{k} = {v:g}" for k, v in p.items())
        raise ValueError(f"the dataset was built with {say(built)}, {who} with {say(expected)}: construct the dataset under "
                         f"the same Config.PCEN settings (infer.py adopts a checkpoint's by itself)")


def checkpoint_payload(epoch, model, optimizer, train_loss, test_loss, feature_statistics=None):
    """The dict format of trainer.py:278-285 (the Config INSTANCE is pickled, as upstream).  ``feature_statistics``: the
    payload of ``standardise_datasets`` (Config.STANDARDISE_FEATURES), stored under that key; None adds no key.
    A capturable Adam keeps its
    learning rate (and step counts) in device tensors; the file holds what the reference's plain Adam would have written --
    a float learning rate, host-side step counts, no ``capturable`` flag -- so that upstream code can format, compare or
    resume from it on any box."""
    opt_state = optimizer.state_dict()
    for group in opt_state.get("param_groups", []):
        if isinstance(group.get("lr"), torch.Tensor):
            group["lr"] = float(group["lr"])
        if group.get("capturable"):
            group["capturable"] = False
    # (state_dict() hands out the LIVE per-parameter state dicts: copy before touching them -- a host-side step count
    # in the running capturable Adam would make its fused kernel dereference a host pointer)
    opt_state["state"] = {k: dict(v) for k, v in opt_state.get("state", {}).items()}
    for entry in opt_state["state"].values():
        if isinstance(entry.get("step"), torch.Tensor):
            entry["step"] = entry["step"].detach().float().cpu()
    if getattr(config, "FEATURE_SET", "logmel") == "logmel_nipd":
        # a pickled instance carries its OWN attributes only: pin what the NIPD channels were computed with, so that
        # infer.py reads them from the file and not from whatever the class says on the day it runs
        for name in NIPD_SETTINGS:
            setattr(config, name, getattr(config, name))
    if getattr(config, "PCEN", False):
        # likewise what the log-mel channels were normalised with; with the switch off no key appears
        for name in PCEN_SETTINGS:
            setattr(config, name, getattr(config, name))
    if getattr(config, "MIC_POSITIONS", None) is not None:
        # likewise the array's geometry: infer.py --tta swaps channels by the positions in the file
        setattr(config, "MIC_POSITIONS", getattr(config, "MIC_POSITIONS"))
    payload = {"epoch": epoch, "model_state_dict": model_state_dict(model),
               "optimizer_state_dict": opt_state, "train_loss": train_loss, "test_loss": test_loss,
               "config": config}
    if float(getattr(config, "EMA_DECAY", 0.0) or 0.0) > 0.0:
        ema = ema_state_dict(model, optimizer)
        if ema is not None:
            payload["ema_state_dict"] = ema
    if feature_statistics is not None:
        payload["feature_statistics"] = feature_statistics
    return payload


def unwrap(model):
    return model.module if isinstance(model, torch.nn.parallel.DistributedDataParallel) else model


# ------------------------------------------------------------------------------------------------
# train_model
# ------------------------------------------------------------------------------------------------

def train_model(train_loader, test_loader, num_epochs=None, batch_size=None, learning_rate=None,
                device=None, use_small_model=True):
    """Complete training run.  Like the reference (trainer.py:36-38) the epoch count, batch size and
    learning rate come from ``config``; the arguments are accepted for signature compatibility."""
    num_epochs, batch_size, learning_rate = config.NUM_EPOCHS, config.BATCH_SIZE, config.LEARNING_RATE
    device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", get_local_rank() if get_world_size() > 1 else torch.cuda.current_device())
    if getattr(config, "SEED", None) is not None:
        torch.manual_seed(config.SEED)
    rank, world = ensure_process_group(device)
    is_main = rank == 0

    train_dataset, test_dataset = train_loader.dataset, test_loader.dataset
    grid = (train_dataset.I, train_dataset.J)
    logger.info(f"Train dataset: {len(train_dataset)} windows ({len(train_loader)} batches)")
    logger.info(f"Test dataset: {len(test_dataset)} windows ({len(test_loader)} batches)")
    logger.info(f"Grid dimensions: {grid[0]}x{grid[1]} = {train_dataset.total_cells} cells; world size {world}")

    # input channels follow the dataset's feature set (4 log-mel; 7 with intensity vectors; 36 for 8-ch GCC-PHAT)
    n_channels = getattr(train_loader.dataset, "n_channels", None)
    model = prepare_model_for_device(build_model(grid, use_small_model, n_channels=n_channels), device)
    n_params = sum(p.numel() for p in model.parameters())
    enable_master_weights(model, device)
    graphed = graph_step_enabled(device, world)
    # captured iterations exchange gradients themselves (bucketed all-reduce between the stage graphs, seld_graph.py); the eager
    # path keeps DistributedDataParallel's bucketed, overlapped reducer
    model = broadcast_replica_state(model, world) if graphed else wrap_ddp(model, device, world)

    class_weights = torch.ones(config.NUM_CLASSES, device=device)
    class_weights[config.NUM_CLASSES - 1] = 0.05            # trainer.py:99-100
    criterion = SMRSELDLoss(loss_type=config.LOSS_TYPE, w_class=config.W_CLASS, w_aiur=config.W_AIUR,
                            w_cl=config.W_CL, grid_size=grid, class_weights=class_weights,
                            three_term=getattr(config, "THREE_TERM_LOSS", False),
                            focal_gamma=getattr(config, "CE_FOCAL_GAMMA", 0.0))
    optimizer = make_optimizer(model, learning_rate, device, capturable=graphed)
    stepper = make_stepper(model, criterion, optimizer, device, world)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=config.LR_DECAY_FACTOR,
                                                           patience=config.LR_DECAY_PATIENCE)
    logger.info(f"Model parameters: {n_params:,}")
    logger.info(f"Optimizer: Adam (lr={learning_rate}, weight_decay={config.WEIGHT_DECAY}); "
                f"ReduceLROnPlateau (factor={config.LR_DECAY_FACTOR}, patience={config.LR_DECAY_PATIENCE})")

    train_feed = make_feed(train_loader, device, rank, world)
    test_feed = make_feed(test_loader, device, rank, world)
    logger.info(f"Batch source: {type(train_feed).__name__}; autocast: {getattr(config, 'AMP_DTYPE', 'fp32')}")
    # Config.STANDARDISE_FEATURES: the training timeline's statistics on both datasets (every rank reduces its own copy of
    # the timeline in the same fixed order: the same bits without a collective); None with the switch off
    feature_statistics = standardise_datasets(train_dataset, test_dataset)
    log_balanced_sampling(train_feed)
    # Config.PCEN: the checkpoints will record this Config's settings, so both datasets must have been built with them
    for ds in (train_dataset, test_dataset):
        check_dataset_pcen(seld_augment.pcen_settings(config), ds, "this run's Config says")

    train_losses, test_losses = [], []
    best_train_loss = best_test_loss = float("inf")
    best_epoch = 0
    stale_epochs = 0
    kept_checkpoints = []
    epoch = 0
    guarded = getattr(optimizer, "guard_active", False)
    skipped_so_far = 0

    for epoch in range(1, num_epochs + 1):
        started = datetime.now()
        # ---- train -----------------------------------------------------------------------------
        model.train()
        loss_sum = torch.zeros((), dtype=torch.float64, device=device)
        term_sum = torch.zeros((), dtype=torch.float64, device=device)
        steps = 0
        static = getattr(stepper, "static_inputs", None) if isinstance(train_feed, DeviceFeed) else None
        if isinstance(train_feed, DeviceFeed):               # the training feed is the only one that augments / balances
            source = train_feed.batches(epoch, out=static, augment=True, balanced=True)
        else:
            source = train_feed.batches(epoch)
        bar = tqdm(source, total=len(train_feed), desc=f"Epoch {epoch}/{num_epochs} [Train]",
                   leave=False, disable=not is_main)
        for spectrograms, labels in bar:
            total, term = stepper(spectrograms, labels)
            loss_sum += total.double()
            term_sum += term.double()
            steps += 1
            if is_main and steps % 25 == 0:
                bar.set_postfix({"loss": f"{total.item():.4f}", "lr": f"{float(optimizer.param_groups[0]['lr']):.6f}"})
        tr_loss, tr_term, tr_steps = all_reduce_sums([loss_sum.item(), term_sum.item(), float(steps)], device)
        avg_train_loss, avg_train_term = tr_loss / max(tr_steps, 1.0), tr_term / max(tr_steps, 1.0)

        # ---- evaluate --------------------------------------------------------------------------
        model.eval()
        loss_sum.zero_()
        term_sum.zero_()
        steps = 0
        with torch.no_grad():
            for spectrograms, labels in tqdm(test_feed.batches(0), total=len(test_feed), leave=False,
                                             desc=f"Epoch {epoch}/{num_epochs} [Test]", disable=not is_main):
                _, total, term = eval_step(model, criterion, spectrograms, labels, device)
                loss_sum += total.double()
                term_sum += term.double()
                steps += 1
        te_loss, te_term, te_steps = all_reduce_sums([loss_sum.item(), term_sum.item(), float(steps)], device)
        avg_test_loss, avg_test_term = te_loss / max(te_steps, 1.0), te_term / max(te_steps, 1.0)

        train_losses.append(avg_train_loss)
        test_losses.append(avg_test_loss)

        old_lr = float(optimizer.param_groups[0]["lr"])
        scheduler.step(avg_test_loss)
        new_lr = float(optimizer.param_groups[0]["lr"])
        if new_lr != old_lr:
            logger.info(f"  Learning rate reduced: {old_lr:.6f} -> {new_lr:.6f}")

        seconds = (datetime.now() - started).total_seconds()
        logger.info(f"\nEpoch {epoch}/{num_epochs} - Duration: {seconds:.1f}s")
        logger.info(f"  Train Loss: {avg_train_loss:.6f} ({config.LOSS_TYPE.upper()}: {avg_train_term:.6f})")
        logger.info(f"  Test Loss:  {avg_test_loss:.6f} ({config.LOSS_TYPE.upper()}: {avg_test_term:.6f})")
        logger.info(f"  Learning Rate: {new_lr:.6f}")
        if guarded:                                   # one device-to-host copy per epoch (the loop above adds no sync)
            report = optimizer.guard_report()
            logger.info(f"  Update guard: grad norm {report['grad_norm']:.4g}, clip coefficient {report['clip_coef']:.4g}, "
                        f"{report['steps_clipped']} clipped / {report['steps_skipped']} skipped updates so far")
            if report["steps_skipped"] > skipped_so_far:
                logger.warning(f"  {report['steps_skipped'] - skipped_so_far} update(s) of this epoch were skipped: "
                               f"non-finite gradient norm")
                skipped_so_far = report["steps_skipped"]

        # early stopping watches the TRAIN loss (trainer.py:262-270)
        if avg_train_loss < best_train_loss - config.MIN_DELTA:
            logger.info(f"  Train loss improved by {best_train_loss - avg_train_loss:.6f}")
            best_train_loss, best_epoch, stale_epochs = avg_train_loss, epoch, 0
        else:
            stale_epochs += 1
            logger.info(f"  No train loss improvement for {stale_epochs} epoch(s)")

        # best checkpoint watches the TEST loss (trainer.py:273-287)
        if avg_test_loss < best_test_loss - config.MIN_DELTA:
            gained = best_test_loss - avg_test_loss
            best_test_loss = avg_test_loss
            if is_main:
                torch.save(checkpoint_payload(epoch, model, optimizer, avg_train_loss, avg_test_loss, feature_statistics),
                           config.CHECKPOINT_PATH / "best_model.pth")
            logger.info(f"  New best model saved! (test loss improvement: {gained:.6f})")

        if epoch % config.SAVE_EVERY_N_EPOCHS == 0 and is_main:
            path = config.CHECKPOINT_PATH / f"checkpoint_epoch_{epoch}.pth"
            torch.save(checkpoint_payload(epoch, model, optimizer, avg_train_loss, avg_test_loss, feature_statistics), path)
            kept_checkpoints.append(path)
            logger.info(f"  Checkpoint saved: {path.name}")
            if len(kept_checkpoints) > config.KEEP_LAST_N_CHECKPOINTS:
                old = kept_checkpoints.pop(0)
                if old.exists():
                    old.unlink()
                    logger.info(f"  Removed old checkpoint: {old.name}")

        if device.type == "cuda" and epoch % 5 == 0:
            torch.cuda.empty_cache()
            gc.collect()

        if stale_epochs >= config.PATIENCE:
            logger.info(f"\nEARLY STOPPING at epoch {epoch}: no train loss improvement for {config.PATIENCE} epochs "
                        f"(best train {best_train_loss:.6f} at epoch {best_epoch}, best test {best_test_loss:.6f})")
            break

    logger.info(f"\nTRAINING COMPLETE: {epoch} epochs, best train loss {best_train_loss:.6f} at epoch {best_epoch}, "
                f"best test loss {best_test_loss:.6f}")

    stamp = datetime.now().strftime("%Y%m%d_%H%M%S")
    if is_main and train_losses:
        plot_loss_curves(train_losses, test_losses, save_path=config.OUTPUT_PATH / f"loss_curves_{stamp}.png")
    if world > 1:
        dist.barrier()
    if hasattr(stepper, "close"):
        logger.info(f"Captured training step: {stepper.stats()}")
        stepper.close()
    disable_master_weights(model)                 # the returned model holds plain fp32 parameters again
    best_path = config.CHECKPOINT_PATH / "best_model.pth"
    if best_path.exists():
        best = safe_torch_load(best_path, map_location=device)
        unwrap(model).load_state_dict(best["model_state_dict"])
        logger.info(f"Best model loaded from epoch {best['epoch']}")

    history = {
        "train_losses": train_losses, "test_losses": test_losses,
        "best_train_loss": best_train_loss, "best_test_loss": best_test_loss,
        "best_epoch": best_epoch, "total_epochs": epoch,
        "config": {"num_epochs": num_epochs, "batch_size": batch_size, "learning_rate": learning_rate,
                   "grid_size": grid,
                   # not upstream: how the epoch was sharded (one process: world 1, every batch on this rank)
                   "world_size": world, "batches_per_rank": len(train_feed), "batch_source": type(train_feed).__name__},
    }
    if is_main:
        history_path = config.OUTPUT_PATH / f"training_history_{stamp}.pth"
        torch.save(history, history_path)
        logger.info(f"Training history saved to {history_path}")
    return unwrap(model), history


# ------------------------------------------------------------------------------------------------
# test_model
# ------------------------------------------------------------------------------------------------

def test_model(test_loader, model_path=None, batch_size=None, device=None, num_visualizations=5,
               save_visualizations=True, use_ema=None):
    """Evaluate a checkpoint (trainer.py:394-711): loss, argmax accuracies, frames with events and a few
    ground-truth-vs-prediction plots.  Accuracies and event counts are reduced on the device batch by
    batch instead of collecting every logit on the host (N x 9 MB x 2 upstream); only the frames that
    are actually plotted are copied back.  Runs on the calling rank only (rank 0 under torchrun)."""
    batch_size = batch_size or config.BATCH_SIZE
    model_path = Path(model_path or (config.CHECKPOINT_PATH / "best_model.pth"))
    device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    test_dataset = test_loader.dataset
    grid = (test_dataset.I, test_dataset.J)
    logger.info(f"Test dataset: {len(test_dataset)} windows ({len(test_loader)} batches)")
    if not model_path.exists():
        raise FileNotFoundError(f"Model checkpoint not found: {model_path}")
    if get_rank() != 0:
        logger.info("test_model runs on rank 0 only")
        return {}

    checkpoint = safe_torch_load(model_path, map_location=device)
    model = prepare_model_for_device(build_model(grid, True, n_channels=getattr(test_dataset, "n_channels", None)),
                                     device)
    model.load_state_dict(select_state_dict(checkpoint, use_ema))
    apply_checkpoint_statistics(checkpoint, test_dataset)      # the checkpoint decides (Config.STANDARDISE_FEATURES)
    check_dataset_pcen(checkpoint_pcen_settings(checkpoint), test_dataset, "the checkpoint records")   # (Config.PCEN)
    model.eval()
    logger.info(f"Model loaded (epoch {checkpoint['epoch']}, test loss {checkpoint['test_loss']:.6f})")
    criterion = SMRSELDLoss(loss_type=config.LOSS_TYPE, w_class=config.W_CLASS, w_aiur=config.W_AIUR,
                            w_cl=config.W_CL, grid_size=grid,          # un-weighted, trainer.py:483-489
                            three_term=getattr(config, "THREE_TERM_LOSS", False),
                            focal_gamma=getattr(config, "CE_FOCAL_GAMMA", 0.0))

    feed = make_feed(test_loader, device, 0, 1)
    bg = config.NUM_CLASSES - 1
    loss_sum = torch.zeros((), dtype=torch.float64, device=device)
    term_sum = torch.zeros((), dtype=torch.float64, device=device)
    correct = torch.zeros((), dtype=torch.int64, device=device)
    correct_events = torch.zeros((), dtype=torch.int64, device=device)
    n_cells = torch.zeros((), dtype=torch.int64, device=device)
    n_events = torch.zeros((), dtype=torch.int64, device=device)
    active_per_frame = []                                     # [B, T] int32 per batch (small)
    steps = 0
    with torch.no_grad():
        for spectrograms, labels in tqdm(feed.batches(0), total=len(feed), desc="Testing"):
            predictions, total, term = eval_step(model, criterion, spectrograms, labels, device)
            loss_sum += total.double()
            term_sum += term.double()
            steps += 1
            pred_cls = predictions.argmax(dim=-1)
            true_cls = _label_classes(labels, config.NUM_CLASSES)
            events = true_cls != bg
            hit = pred_cls == true_cls
            correct += hit.sum()
            correct_events += (hit & events).sum()
            n_cells += hit.numel()
            n_events += events.sum()
            active_per_frame.append(events.sum(dim=-1).to(torch.int32).cpu())
    avg_test_loss = loss_sum.item() / max(steps, 1)
    avg_test_term = term_sum.item() / max(steps, 1)
    overall_accuracy = 100.0 * correct.item() / max(n_cells.item(), 1)
    non_bg_accuracy = 100.0 * correct_events.item() / n_events.item() if n_events.item() > 0 else 0.0
    logger.info(f"Total Loss: {avg_test_loss:.6f}  (Class {config.LOSS_TYPE.upper()}: {avg_test_term:.6f})")
    logger.info(f"Overall Accuracy: {overall_accuracy:.2f}%  Non-Background Accuracy: {non_bg_accuracy:.2f}%")
    logger.info(f"Active Events: {n_events.item()} / {n_cells.item()}")

    active = torch.cat(active_per_frame, dim=0) if active_per_frame else torch.zeros((0, 0), dtype=torch.int32)
    frames_with_events = [(int(w), int(t), int(active[w, t])) for w, t in (active > 0).nonzero().tolist()]
    logger.info(f"Found {len(frames_with_events)} frames with active events")
    results = {
        "test_loss": avg_test_loss, f"class_{config.LOSS_TYPE}": avg_test_term,
        "overall_accuracy": overall_accuracy, "non_bg_accuracy": non_bg_accuracy,
        "num_frames_with_events": len(frames_with_events), "visualizations": [],
        "checkpoint_epoch": checkpoint["epoch"],
    }
    if not frames_with_events:
        logger.warning("No frames with active events found! Cannot create visualizations.")
        return results

    chosen = random.sample(frames_with_events, min(num_visualizations, len(frames_with_events)))
    chosen.sort(key=lambda f: f[2], reverse=True)
    if save_visualizations:
        (config.OUTPUT_PATH / "test_visualizations").mkdir(exist_ok=True)
    for viz, (window_idx, time_idx, num_active) in enumerate(chosen, start=1):
        spec, labels = test_dataset[window_idx]
        spec = spec.unsqueeze(0).to(device)
        if getattr(test_dataset, "feature_stats", None) is not None:     # __getitem__ stays raw: the model's input is the
            spec = test_dataset.device_batch([window_idx])[0]            # standardised window of the device gather
        with torch.no_grad(), autocast_context(device):
            logits = model(spec)[0, time_idx].float().cpu()
        save_path = None
        if save_visualizations:
            save_path = config.OUTPUT_PATH / "test_visualizations" / f"test_viz_{viz}_window{window_idx}_frame{time_idx}.png"
        fig = visualize_grid_predictions(ground_truth=labels[time_idx], predictions=logits, time_frame=time_idx,
                                         grid_size=grid, title_prefix=f"Window {window_idx}, ", save_path=save_path)
        results["visualizations"].append({"window_idx": window_idx, "time_idx": time_idx, "num_active": num_active,
                                          "figure": fig, "save_path": save_path})
    logger.info("TESTING COMPLETE")
    return results


# ------------------------------------------------------------------------------------------------
# evaluate_seld: detections and SELD metrics (no reference counterpart; seld_eval.py)
# ------------------------------------------------------------------------------------------------

def timeline_logits(model, dataset, batch_size, device, patterns=None):
    """The model's logits [B, 250, 648, 14] for every window of ``dataset`` in timeline order, one batch at a time (eval
    mode is the caller's; autocast as in training).  Windows come from the device timeline when the dataset keeps one.
    ``patterns``: a non-empty list of spatial patterns (test-time augmentation) yields
    [P, B, 250, 648, 14] instead: every batch of windows is gathered once per pattern by the augmenting gather (channel
    table row of the pattern, no masks; its permuted labels are not used) and the model runs once per pattern on a batch
    of the usual size, into one buffer that is reused from batch to batch -- a yielded tensor is valid until the next
    one is asked for.  Needs the device timeline (no CPU fallback)."""
    on_device = device.type == "cuda" and getattr(dataset, "spec_tm", None) is not None
    patterns = seld_augment.tta_patterns(patterns, array=getattr(dataset, "mic_array", None))
    if not patterns:
        return _plain_logits(model, dataset, batch_size, device, on_device)
    if not on_device:
        raise RuntimeError("test-time augmentation gathers its windows on the GPU: it needs a ROCm device and a dataset "
                           "that keeps its device timeline (keep_on_device=True); there is no CPU fallback")
    return _tta_logits(model, dataset, batch_size, device, patterns)


def _plain_logits(model, dataset, batch_size, device, on_device):
    n = len(dataset)
    for lo in range(0, n, batch_size):
        idx = list(range(lo, min(lo + batch_size, n)))
        if on_device:
            spec, _ = dataset.device_batch(idx)
        else:
            spec = torch.stack([dataset[i][0] for i in idx]).to(device)
        with torch.no_grad(), autocast_context(device):
            logits = model(spec)
        yield logits


def _tta_logits(model, dataset, batch_size, device, patterns):
    n = len(dataset)
    stacks = None
    for lo in range(0, n, batch_size):
        idx = list(range(lo, min(lo + batch_size, n)))
        for k, p in enumerate(patterns):
            spec, _ = dataset.device_batch(idx, augment=seld_augment.tta_rows(p, len(idx)))
            with torch.no_grad(), autocast_context(device):
                logits = model(spec)
            if stacks is None:
                stacks = torch.empty((len(patterns), min(batch_size, n)) + tuple(logits.shape[1:]), dtype=logits.dtype,
                                     device=logits.device)
            stacks[k, :len(idx)] = logits
        yield stacks[:, :len(idx)]


def evaluate_seld(test_loader, model_path=None, batch_size=None, device=None, threshold=None, max_peaks=None,
                  doa_threshold_deg=None, events_dir=None, use_ema=None, tta=None, track=None, refine=None, sweep=None,
                  class_thresholds=None, thresholds_out=None, segment=None, jackknife=None):
    """Evaluate a checkpoint on what it detects: the windows of ``test_loader.dataset`` (an SELDDataset) run through the
    model in timeline order, the overlapping grid maps are decoded into DOA events on the GPU and scored against the
    dataset's CSV rows.  Returns F20, ER20, LE_CD, LR_CD, TP, FP, FN, N, per_class (seld_eval.evaluate_logits); with
    ``events_dir`` one event CSV per file, named after its audio stem.  The checkpoint is loaded as test_model loads it;
    runs on rank 0 only.
    ``tta``: the spatial patterns of test-time augmentation (seld_augment.tta_patterns: "all", a list, or () for off;
    None reads Config.SELD_TTA_PATTERNS): the model runs on every transformed copy of a window and the un-permuted grid
    maps are averaged before the peak test; the result's "tta_patterns" lists them.
    ``track``: track linking of the detections (seld_eval.evaluate_logits: None reads Config.SELD_TRACK, True or a dict
    of gate_deg / max_gap / min_len switches it on); the result's "tracking" holds its counts.
    ``refine``: sub-cell DOA refinement of the detections (seld_eval.evaluate_logits: None reads Config.SELD_REFINE;
    DESIGN.md section 15); the result's "refine" says whether the scored and written directions are refined.
    ``sweep`` / ``class_thresholds`` / ``thresholds_out``: the threshold sweep, per-class detection thresholds and the
    thresholds file of seld_eval.evaluate_logits (None reads Config.SELD_SWEEP_THRESHOLDS /
    SELD_CLASS_THRESHOLDS / SELD_THRESHOLDS_OUT).  ``sweep`` also takes the spelling "0.05:0.95:0.05" (start:stop:step,
    inclusive) or a comma list; the one forward pass and the one decode serve every threshold, the result's "sweep"
    holds a record per threshold and the best global / per-class operating points.
    ``segment`` / ``jackknife``: the segment-based, class-macro metrics of seld_eval.evaluate_logits (DESIGN.md section 18;
    None reads Config.SELD_SEGMENT_METRICS / SELD_JACKKNIFE): the result's "segment" holds micro and macro F, ER, LE, LR and
    the SELD score per 1 s block and class, with ``jackknife`` also their 95 % confidence intervals over the recordings."""
    import seld_eval
    seld_eval.segment_setting(segment, jackknife)          # (jackknife without segment: raise before the checkpoint is read)
    test_dataset = test_loader.dataset
    # a dataset of a microphone array (Config.MIC_POSITIONS): "all" = the array's symmetries
    array = getattr(test_dataset, "mic_array", None)
    patterns = seld_augment.tta_patterns(getattr(config, "SELD_TTA_PATTERNS", ()) if tta is None else tta, array=array)
    seld_augment.check_tta(patterns, getattr(config, "FEATURE_SET", "logmel"), getattr(test_dataset, "n_channels", 0),
                           array=array)
    batch_size = batch_size or getattr(test_loader, "batch_size", None) or config.BATCH_SIZE
    model_path = Path(model_path or (config.CHECKPOINT_PATH / "best_model.pth"))
    device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if not model_path.exists():
        raise FileNotFoundError(f"Model checkpoint not found: {model_path}")
    if get_rank() != 0:
        logger.info("evaluate_seld runs on rank 0 only")
        return {}
    checkpoint = safe_torch_load(model_path, map_location=device)
    model = prepare_model_for_device(build_model((test_dataset.I, test_dataset.J), True,
                                                 n_channels=getattr(test_dataset, "n_channels", None)), device)
    model.load_state_dict(select_state_dict(checkpoint, use_ema))
    apply_checkpoint_statistics(checkpoint, test_dataset)      # the checkpoint decides (Config.STANDARDISE_FEATURES)
    check_dataset_pcen(checkpoint_pcen_settings(checkpoint), test_dataset, "the checkpoint records")   # (Config.PCEN)
    model.eval()
    logger.info(f"SELD evaluation: {len(test_dataset)} windows, checkpoint epoch {checkpoint['epoch']}")
    if patterns:
        logger.info(f"test-time augmentation: {len(patterns)} forwards per window, spatial patterns {list(patterns)}")
    results = seld_eval.evaluate_logits(timeline_logits(model, test_dataset, batch_size, device, patterns=patterns),
                                        test_dataset, threshold=threshold, max_peaks=max_peaks,
                                        doa_threshold_deg=doa_threshold_deg, events_dir=events_dir, patterns=patterns,
                                        track=track, refine=refine, sweep=sweep, class_thresholds=class_thresholds,
                                        thresholds_out=thresholds_out, segment=segment, jackknife=jackknife)
    results["checkpoint_epoch"] = checkpoint["epoch"]
    if results.get("sweep"):
        sw = results["sweep"]
        for t, f, e in zip(sw["thresholds"], sw["F20"], sw["ER20"]):
            logger.info(f"threshold {t:.4g}: F20 {f:.4f}  ER20 {e:.4f}")
        logger.info(f"best threshold {sw['best']['global']}, per class {sw['best']['per_class']}"
                    + (f" -> {results['thresholds_file']}" if results.get("thresholds_file") else ""))
    if results.get("tracking"):
        tr = results["tracking"]
        logger.info(f"track linking (gate {tr['gate_deg']:g} deg, gap {tr['max_gap']}, min length {tr['min_len']}): "
                    f"{tr['tracks_kept']} of {tr['tracks']} tracks kept, {tr['filled']} frames filled")
    logger.info(f"F20 {results['F20']:.4f}  ER20 {results['ER20']:.4f}  LE_CD {results['LE_CD']:.2f} deg  "
                f"LR_CD {results['LR_CD']:.4f}  (TP {results['TP']}, FP {results['FP']}, FN {results['FN']}, "
                f"N {results['N']})")
    if results.get("segment"):
        sg = results["segment"]
        for avg in ("micro", "macro"):
            m = sg[avg]
            logger.info(f"segment-based {avg}: F {m['F']:.4f}  ER {m['ER']:.4f}  LE {m['LE']:.2f} deg  LR {m['LR']:.4f}  "
                        f"SELD {m['SELD']:.4f}"
                        + (f"  (95 % CI of SELD {sg['ci'][avg]['SELD']['low']:.4f} .. {sg['ci'][avg]['SELD']['high']:.4f}, "
                           f"{sg['ci'][avg]['SELD']['n']} recordings)" if "ci" in sg else ""))
    return results


def _label_classes(labels, num_classes):
    """argmax over classes of the labels, for dense float labels or the compact uint16 mask
    (lowest set bit = first maximal class, as torch.argmax picks the first maximum; mask 0 = background)."""
    if labels.dtype != torch.uint16:
        return labels.argmax(dim=-1)
    m = labels.to(torch.int32)
    lowest = (m & -m).float().log2().to(torch.int64)
    return torch.where(m == 0, torch.full_like(lowest, num_classes - 1), lowest)
