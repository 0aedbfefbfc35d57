"""The case table of tests/test_second_lap_gpu.py: one entry per launch site of csrc/ that sizes its grid from the device's
CU count, at the smallest shape that makes the kernel walk its grid-stride (or persistent) loop at least three times when
the library sees ONE compute unit (SELD_CUS=1, read by seld_init).  Importable without a GPU and without torch.

An entry names the entry point, the shape, the launch sites it covers (file + a piece of the source line that reads
``num_cus``: what tests/test_second_lap_cases_cpu.py matches the source against), the reference that judges it with the bar
the kernel's own test module applies, and ``launches``: the host's arithmetic restated -- work items, items per workgroup
and the grid -- with the file:line it restates.  ``laps`` / ``ragged`` below are what the CPU test asserts of every launch.

A launch is ``(label, items, per_group, grid)``: ``grid`` workgroups (or wavefronts, where the host deals whole wavefronts)
of ``per_group`` items stride over ``items``; a group walks ceil(ceil(items / per_group) / grid) laps at the most, and the
last lap is ragged when the items do not fill it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def laps(launch) -> int:
    _, items, per_group, grid = launch
    return cdiv(cdiv(items, per_group), grid)


def ragged(launch) -> bool:
    """The last lap is not a full one: some group has no item in it, or the last item is partial."""
    _, items, per_group, grid = launch
    return items % (per_group * grid) != 0


def frames_of(samples: int) -> int:
    return 1 + samples // 480


@dataclass(frozen=True)
class Case:
    name: str
    entry: str                      # the seld_native function / C symbol driven
    shape: dict
    sites: tuple                    # ((file, piece of the line that reads num_cus), ...)
    launches: Callable              # (shape, num_cus) -> [(label, items, per_group, grid), ...]
    judge: str                      # the reference and the bar, as the kernel's own test module has them
    bit_equal: bool = False


# ---- the caps, restated -----------------------------------------------------------------------------------------------

def class_loss_blocks(n_cells, num_cus):
    """loss_core.h:247 class_loss_blocks: eight blocks per CU, no more than tiles or kLossMaxPartials = 4096."""
    tiles = cdiv(n_cells, 256)
    return min(num_cus * 8, tiles, 4096)


def grid_for(work_items, block, num_cus):
    """labels.hip:133 grid_for"""
    return max(1, min(cdiv(work_items, block), num_cus * 8))


def window_grid(per_window, B, num_cus):
    """augment_core.h:190 window_grid -> (x, y): x blocks stride over one window's chunks, y = one row of blocks per window"""
    x = cdiv(per_window, 256)
    cap = num_cus * 32
    y = min(B, 65535)
    if x * y > cap:
        x = cdiv(cap, y)
    return max(x, 1), y


def _class_loss(shape, num_cus):
    n = shape["n_cells"]
    return [("256-cell tiles", n, 256, class_loss_blocks(n, num_cus))]          # loss.hip / loss_ce.hip: tile loop


def _smr_loss(shape, num_cus):
    out = []
    for frames, grid in shape["grids"]:
        n = frames * grid[0] * grid[1]
        out.append((f"{frames} x {grid}", n, 256, class_loss_blocks(n, num_cus)))      # loss3.hip:122 tile loop
    return out


def _scale(shape, num_cus):
    n8 = shape["n"] // 8                                                          # loss.hip:127-130
    return [("8-element pieces", n8, 256, min(cdiv(n8, 256), num_cus * 8))]


def _expand(shape, num_cus):
    q = shape["n_cells"] * 14 // 4                                                # labels.hip:196: one float4 per thread
    return [("float4 stores", q, 256, grid_for(q, 256, num_cus))]


def _gather_rows(shape, num_cus):
    q = shape["B"] * shape["window"] * shape["row_bytes"] // 16                   # labels.hip:212 / :229: 16-byte chunks
    return [("16-byte chunks", q, 256, grid_for(q, 256, num_cus))]


def _window_features(shape, num_cus):
    per_window = shape["window"] * shape["channels"] * 16                         # window * row_chunks (augment.hip:129 ...)
    x, _ = window_grid(per_window, shape["B"], num_cus)
    return [("chunks of one window", per_window, 256, x)]


def _window_mask(shape, num_cus):
    per_window = shape["window"] * (shape["cells"] // 8)                          # augment.hip:150, mix.hip:313
    x, _ = window_grid(per_window, shape["B"], num_cus)
    return [("mask chunks of one window", per_window, 256, x)]


def _window_features_and_mask(shape, num_cus):
    return _window_features(shape, num_cus) + _window_mask(shape, num_cus)


def _mix(shape, num_cus):
    out = _window_features(shape, num_cus)                                        # mix.hip:264 mix_chunks
    if shape.get("iv_channels"):
        per_window = shape["window"] * 16                                         # mix.hip:272 mix_units: kChunksPerChannel
        x, _ = window_grid(per_window, shape["B"], num_cus)
        out.append(("intensity units of one window", per_window, 256, x))
    return out + _window_mask(shape, num_cus)


def _frame_mask(shape, num_cus):
    groups = cdiv(shape["rows"], 4)                                               # balance.hip:138 kFrameGroup = 4
    want = cdiv(groups, 4)                                                        # :139 kFrameWaves = 4
    blocks = min(want, num_cus * 8)                                               # :140
    return [("groups of four rows, per wavefront", groups, 1, blocks * 4)]


def _window_count(shape, num_cus):
    n = shape["n_windows"]
    return [("windows", n, 1, min(n, num_cus * 32))]                              # balance.hip:169


def _balance(shape, num_cus):
    return _frame_mask(shape, num_cus) + _window_count(shape, num_cus)


def _moments(shape, num_cus):
    slabs = cdiv(shape["rows"], 1024)                                             # standardise.hip:89 kSlabFrames = 1024
    tiles = cdiv(shape["channels"] * 16, 64)                                      # :120
    items = slabs * tiles
    return [("slab tiles", items, 1, min(items, num_cus * 32))]                   # :124


def _pcen(shape, num_cus):
    chunks = cdiv(shape["T"], 256)                                                # pcen.hip:191 kPcenChunk = 256
    tiles = cdiv(shape["C_log"] * 16, 64)                                         # :246
    walked = chunks - 1 if chunks > 1 else 1                                      # :247
    carry, apply_ = shape["N"] * walked * tiles, shape["N"] * chunks * tiles      # :249
    cap = num_cus * 32                                                            # :248
    return [("carry items", carry, 1, min(carry, cap)), ("apply items", apply_, 1, min(apply_, cap))]


def _mix_all(shape, num_cus):
    out = []
    for channels, iv in shape["sets"]:
        for launch in _mix(dict(shape, channels=channels, iv_channels=iv), num_cus)[:-1]:
            out.append((f"C = {channels}: {launch[0]}",) + launch[1:])
    return out + _window_mask(shape, num_cus)


def _mic_all(shape, num_cus):
    out = []
    for kind, channels in shape["kinds"]:
        units = cdiv(shape["window"], 4) * channels                               # micswap.hip:172: four frames per wavefront
        x, _ = window_grid(units * 64, shape["B"], num_cus)                        # :173
        out.append((f"{kind}: (four frames, channel) units, four per block", units, 4, x))
    return out


def _frames(shape):
    return shape["N"] * frames_of(shape["L"])


def _per_frame(waves, cap_per_cu):
    def launches(shape, num_cus):
        frames = _frames(shape)
        blocks = min(cdiv(frames, waves), num_cus * cap_per_cu)                   # rotate.hip:291, spatial.hip:983, nipd.hip:223
        return [("frames, one per wavefront", frames, 1, blocks * waves)]
    return launches


def _iter_geometry(L):
    """logmel_core.h:69 iter_geometry -> (F, iters_per_row, interior)"""
    F = frames_of(L)
    iters = cdiv(F, 4)
    interior = min(max((L // 480 - 4) // 4, 0), iters - 1)
    return F, iters, interior


def _logmel_main(shape, num_cus):
    _, iters, interior = _iter_geometry(shape["L"])
    rows = shape["N"] * shape["C"]
    n_edge, total = rows * (iters - interior), rows * interior                   # logmel.hip:495
    reserve = min(cdiv(cdiv(n_edge, 8), 8), 4)                                    # :506
    cus = max(num_cus - reserve, 1)                                               # :509
    waves = min(cdiv(total, 8), cus * 8)                                          # :511 kMainWaves = 8
    chunk = cdiv(total, waves)                                                    # :514 a wavefront's contiguous run
    return [("interior iterations, a contiguous run per wavefront", total, 1, cdiv(total, chunk))]


def _stft(shape, num_cus):
    _, iters, _ = _iter_geometry(shape["L"])
    total = shape["N"] * shape["C"] * iters                                       # logmel.hip:452
    waves = min(cdiv(total, 4), num_cus * 8)                                      # :453
    chunk = cdiv(total, waves)
    return [("iterations, a contiguous run per wavefront", total, 1, cdiv(total, chunk))]


def _logmel_iv(shape, num_cus):
    F, iters, _ = _iter_geometry(shape["L"])
    total = shape["N"] * iters                                                    # logmel.hip:436
    groups = min(total, num_cus)                                                  # :437
    chunk = cdiv(total, groups)
    # in frames: an iteration is four frames and a clip's last one is partial (F % 4 != 0)
    assert cdiv(shape["N"] * F, 4) == total
    return [("frames, four per iteration, a contiguous run per workgroup", shape["N"] * F, 4, cdiv(total, chunk))]


def _gcc(shape, num_cus):
    frames = _frames(shape)
    return [("mfma / planar: frame pairs", frames, 2, min(cdiv(frames, 2), num_cus)),           # spatial.hip:1018, :1058
            ("q15: groups of kGqFrames = 4 frames", frames, 4, min(cdiv(frames, 4), num_cus)),  # :1023
            ("fft: frames", frames, 1, min(frames, num_cus * 4))]                               # :1067


def _tail(shape, num_cus):
    out = []
    for mode, c, _ in shape["cases"]:
        per_block = 256 // (c // 8)                                               # convtail.hip:441 kTailThreads = 256
        out_rows = tail_rows(mode, c, num_cus)[1]
        out.append((f"mode {mode} C = {c}: output rows", out_rows, per_block, min(cdiv(out_rows, per_block), num_cus * 8)))
    return out


def tail_rows(mode, c, num_cus):
    """(rows, out_rows) of tests/test_tail_parity_gpu.py test_unrolled_main_loops_are_reached for a device of num_cus: every
    slot runs the two-in-flight loop once, the first P + 1 slots the remainder loop, the rest nothing."""
    g, p = 8 * num_cus, 2048 // c
    out_rows = 2 * g * p + p + 1
    if mode == 2:
        out_rows += out_rows % 2
    return (2 * out_rows if mode == 2 else out_rows), out_rows


def _convfirst(shape, num_cus):
    out = []
    for b, t, f in shape["shapes"]:
        chunks = b * cdiv(t, 256 // f)                                            # convfirst.hip:716-722 kCfPos = 256
        groups = min(2 * num_cus, 512, chunks)                                    # :728
        out.append((f"{(b, t, f)}: chunks", chunks, 1, groups))
    return out


def _wgrad(shape, num_cus):
    out = []
    for b, cin, cout, t, f in shape["shapes"]:
        tc = 128 // f                                                             # convwgrad.hip:247 kWgKc = 128
        chunks = b * cdiv(t, tc)
        tiles = (cin // 64) * (cout // 64)
        slabs = max(1, min(cdiv(num_cus, tiles), chunks))                         # :261-262
        # one CU: one slab holds the whole K, its workgroups walk the clips one after the other; per clip:
        out.append((f"{(b, cin, cout, t, f)}: time rows of one clip, {tc} per chunk, {b} clips per slab", t, tc, slabs))
    return out


FRONT = {"N": 3, "C": 4, "L": 24000}        # 3 clips of 51 frames = 13 iterations (11 interior), the last one of 3 frames

LOSS_JUDGE = ("float64 torch softmax + MSE on the logits as the kernel sees them; value 1e-5 relative, gradient 1e-5 (fp32) / "
              "8e-3 (bf16) of max(1, |g|max): tests/test_loss_gpu.py")

CASES = [
    # ---- class losses: all eight instantiations (bf16 / fp32 x mask / dense x value / value + gradient) each
    Case("softmax_mse", "seld_native.softmax_mse", {"n_cells": 19 * 256 + 5},
         (("loss_core.h", "long blocks = static_cast<long>(st->num_cus) * 8;"),), _class_loss, LOSS_JUDGE),
    Case("softmax_ce", "seld_native.softmax_ce", {"n_cells": 19 * 256 + 5, "gammas": (0.0, 2.0)},
         (("loss_core.h", "long blocks = static_cast<long>(st->num_cus) * 8;"),), _class_loss,
         "tests/loss_ce_ref.py (float64); value 1e-5, W 1e-7 relative, gradient 1e-4 (fp32) / 8e-3 (bf16) of |g|max: "
         "tests/test_loss_ce_gpu.py"),
    # 18 x 36: the product grid (a tile spans two frames); 3 x 3 over 700 frames: the straight-to-global counter branch;
    # 16 x 16 = exactly 256 cells and 32 x 32 = kL3MaxCells: either side of `cells_per_frame >= 256`, tiles on frame edges
    Case("smr_loss", "seld_native.smr_loss",
         {"grids": ((7, (18, 36)), (700, (3, 3)), (17, (16, 16)), (5, (32, 32)), (150, (5, 7)))},
         (("loss_core.h", "long blocks = static_cast<long>(st->num_cus) * 8;"),), _smr_loss,
         "_three_term_reference of tests/test_loss_gpu.py in float64; terms 2e-5 of max(1, |terms|max), gradient 1e-4 (fp32) / "
         "8e-3 (bf16) of |g|max"),
    Case("scale_by_scalar", "seld_native.scale_by_device_scalar_", {"n": 8 * (19 * 256 + 5)},
         (("loss.hip", "const long cap = static_cast<long>(st->num_cus > 0 ? st->num_cus : 256) * 8;"),), _scale,
         "float64 product; 1e-4 (fp32) / 1e-2 (bf16) of the largest element: the bars of "
         "test_module_backward_with_and_without_upstream_scale"),
    # ---- labels and the plain gathers: bit-equal
    Case("expand_labels", "seld_native.expand_labels", {"n_cells": 27 * 648},
         (("labels.hip", "const unsigned blocks = grid_for(n_cells * num_classes / 4, 256, st->num_cus);"),
          ("labels.hip", "static unsigned grid_for(long work_items, int block, int num_cus) {"),
          ("labels.hip", "const long cap = static_cast<long>(num_cus) * 8;")), _expand,
         "oracle/labels.py mask_to_dense: bit-equal", bit_equal=True),
    Case("gather_rows", "seld_native.gather_windows", {"B": 5, "window": 37, "row_bytes": 648 * 2, "rows": 120},
         (("labels.hip", "const unsigned blocks = grid_for(B * window * chunks, 256, st->num_cus);"),), _gather_rows,
         "oracle/windows.py make_window_mask on uint16 mask rows (tail-padded, all-padding and repeated windows): bit-equal",
         bit_equal=True),
    Case("gather_rows_affine", "seld_native.gather_windows_affine", {"B": 5, "window": 37, "row_bytes": 5 * 256, "rows": 120},
         (("labels.hip", "const unsigned blocks = grid_for(B * window * chunks, 256, st->num_cus);"),), _gather_rows,
         "power-of-two scales: tests/standardise_ref.py affine_exact_scale of the oracle's windows, bit-equal, padding exactly +0.0",
         bit_equal=True),
    # ---- window-grid gathers
    Case("gather_augment", "seld_native.gather_windows_augment + gather_windows_permute",
         {"B": 5, "window": 250, "channels": 7, "cells": 648, "rows": 640},
         (("augment.hip", "gather_augment_kernel<kAffine>, window_grid(window * row_chunks, B, st->num_cus)"),
          ("augment.hip", "permute_mask_kernel<kStep>, window_grid(window * (cells / 8), B, st->num_cus)"),
          ("augment_core.h", "static inline dim3 window_grid(long per_window, long B, int num_cus) {"),
          ("augment_core.h", "const long cap = static_cast<long>(num_cus) * 32;")), _window_features_and_mask,
         "tests/augment_ref.py gather: features and labels bit-equal", bit_equal=True),
    Case("gather_rotate", "seld_native.gather_windows_rotate + gather_windows_permute_rotate",
         {"B": 16, "window": 50, "channels": 7, "cells": 648},
         (("rotate.hip", "gather_rotate_kernel<kAffine>, window_grid(per_window, B, st->num_cus)"),
          ("augment.hip", "permute_mask_kernel<kStep>, window_grid(window * (cells / 8), B, st->num_cus)")),
         _window_features_and_mask,
         "tests/rotate_ref.py gather in float64 on the device's own timeline and terms, its per-element bounds; copied, masked and "
         "zero elements and the labels bit-equal: test_rotated_windows_match_the_formulas_in_float64"),
    Case("gather_mic", "seld_native.gather_windows_mic", {"B": 12, "window": 18, "kinds": (("nipd", 7), ("gcc", 10))},
         (("micswap.hip", "gather_mic_kernel<kAffine>, window_grid(units * 64, B, st->num_cus)"),), _mic_all,
         "tests/mic_swap_ref.py gather (tetrahedron, with and without the affine map): bit-equal", bit_equal=True),
    # B = 32 windows: one block per window, so that the 800 intensity units of a window are four laps
    Case("gather_mix", "seld_native.gather_windows_mix + gather_windows_mix_mask",
         {"B": 32, "window": 50, "sets": ((4, 0), (7, 3)), "cells": 648},
         (("mix.hip", "mix_chunks_kernel<kAffine>, window_grid(window * row_chunks, B, st->num_cus)"),
          ("mix.hip", "mix_units_kernel<kAffine>, window_grid(window * kChunksPerChannel, B, st->num_cus)"),
          ("mix.hip", "mix_mask_kernel, window_grid(window * (cells / 8), B, st->num_cus)")), _mix_all,
         "tests/mix_ref.py gather in float64 with its per-element bounds; copied and masked elements bit-equal to the "
         "restatement, labels bit-equal: test_mixed_frames_match_the_restatement_in_float64"),
    Case("spectral", "seld_native.window_spectral", {"B": 8, "window": 50, "channels": 7},
         (("spectral.hip", "spectral_kernel<kAffine>, window_grid(window * row_chunks, B, st->num_cus)"),), _window_features,
         "tests/spectral_ref.py stage, every window with a shift, a curve, cutouts and masks, in place: bit-equal", bit_equal=True),
    # ---- timeline passes
    Case("balance", "seld_frame_class_mask + seld_window_class_frames", {"rows": 613, "n_windows": 205, "window": 7, "hop": 3},
         (("balance.hip", "const int64_t cap = static_cast<int64_t>(st->num_cus) * 8;"),
          ("balance.hip", "const int64_t cap = static_cast<int64_t>(st->num_cus) * 32;")), _balance,
         "tests/balance_ref.py: bit-equal, sentinels behind the outputs untouched", bit_equal=True),
    # (the one tensor above the low megabytes: a slab is 1024 frames and 32 one-wave blocks need 65 of them; one channel)
    Case("feature_moments", "seld_native.feature_moments", {"rows": 64 * 1024 + 3, "channels": 1},
         (("standardise.hip", "const int64_t cap = static_cast<int64_t>(st->num_cus) * 32;"),), _moments,
         "tests/standardise_ref.py moments: bit-equal (fixed-order double sums per slab, folded in slab order)", bit_equal=True),
    Case("pcen", "seld_native.pcen", {"N": 3, "T": 11 * 256 + 7, "C_log": 5, "C_total": 6},
         (("pcen.hip", "const int64_t cap = static_cast<int64_t>(st->num_cus) * 32;"),), _pcen,
         "tests/pcen_ref.py ref64; error factor <= DEVICE_FACTOR * REF32_K of the setting; the other channels bit-equal copies"),
    # ---- front end: three clips, so that clip boundaries, a silent channel and an all-zero frame fall into later laps
    Case("logmel", "seld_native.logmel", FRONT,
         (("logmel.hip", "long cus = static_cast<long>(st->num_cus) - reserve;"),), _logmel_main,
         "oracle/features.py logmel_torch through tests/logmel_checks.py assert_logmel_close (1e-4 dB on the strong bands)"),
    Case("stft", "seld_native.stft", FRONT,
         (("logmel.hip", "const long max_waves = static_cast<long>(st->num_cus) * 8;"),), _stft,
         "oracle/features.py stft_f64: 2e-6 of the largest magnitude (tests/test_spatial_gpu.py)"),
    Case("logmel_iv", "seld_native.spatial_features('logmel_iv')", FRONT,
         (("logmel.hip", "long groups = total < st->num_cus ? total : static_cast<long>(st->num_cus);"),), _logmel_iv,
         "log-mel channels: assert_logmel_close; intensity vectors: oracle/features.py foa_intensity_f64 within 1e-4"),
    Case("foa_iv", "seld_native.spatial_features('logmel_iv') under SELD_FOA=spectra", FRONT,
         (("spatial.hip", "const long cap = static_cast<long>(st->num_cus) * 8;"),), _per_frame(4, 8),
         "oracle/features.py foa_intensity_f64 within 1e-4"),
    Case("gcc_phat", "seld_native.spatial_features('logmel_gcc') under SELD_GCC = mfma, planar, spectra, fft", FRONT,
         (("spatial.hip", "if (blocks > st->num_cus) blocks = st->num_cus;"),
          ("spatial.hip", "const long cap = static_cast<long>(st->num_cus) * 4;")), _gcc,
         "oracle/features.py gcc_phat_f64 within 1e-4; pairs with the silent channel and the all-zero frame: the unit pulse "
         "within 2e-5, the frame's log-mel exactly -100 dB (tests/test_spatial_gpu.py, DESIGN.md 7.5)"),
    Case("nipd", "seld_native.nipd_q15", FRONT,
         (("nipd.hip", "const long cap = static_cast<long>(st->num_cus) * 8;"),), _per_frame(4, 8),
         "tests/nipd_ref.py nipd_from_words on the device's own words: 1e-5 m"),
    Case("rotation_terms", "seld_native.foa_rotation_terms", FRONT,
         (("rotate.hip", "const long cap = static_cast<long>(st->num_cus) * 8;"),), _per_frame(4, 8),
         "tests/rotate_ref.py rotation_terms_f64: powers 1e-4 dB on the strong elements, cross term 2.3e-5 sqrt(P_X P_Y)"),
    # ---- encoder
    Case("conv_tail", "seld_native.conv_tail_forward / conv_tail_backward",
         {"cases": ((2, 64, "bf16"), (1, 1024, "bf16"), (3, 2048, "bf16"), (4, 512, "bf16"), (1, 1024, "fp32"), (4, 512, "fp32"))},
         (("convtail.hip", "const long cap = static_cast<long>(st->num_cus > 0 ? st->num_cus : 256) * 8;"),), _tail,
         "tests/tail_checks.py run_checks (float64 replay from the kernel's own coefficients): every ratio <= 1"),
    Case("convfirst", "seld_native.convfirst_forward / convfirst_backward", {"shapes": ((3, 9, 64), (1, 7, 256))},
         (("convfirst.hip", "int groups = 2 * (st->num_cus > 0 ? st->num_cus : 256);"),), _convfirst,
         "tests/convfirst_checks.py run_checks at the plan of one CU, both families: every ratio <= 1, y and dbeta bit-equal"),
    Case("conv3x3_wgrad", "seld_native.conv3x3_wgrad", {"shapes": ((3, 64, 64, 37, 8), (3, 128, 64, 21, 16), (2, 64, 128, 11, 32))},
         (("convwgrad.hip", "WgradPlan wgrad_plan(int64_t B, int64_t T, int64_t F, int64_t Cin, int64_t Cout, int num_cus) {"),
          ("convwgrad.hip", "const long want = ((num_cus > 0 ? num_cus : 256) + tiles - 1) / tiles;"),
          ("convwgrad.hip", "wgrad_plan(B, T, F, Cin, Cout, st->num_cus)")), _wgrad,
         "float64 aten.convolution_backward on the host; 1e-5 of the magnitude sum + one bf16 rounding for a bf16 gradient: the "
         "bound of tests/test_conv_wgrad_gpu.py"),
]

# Lines of csrc/ that read num_cus without sizing a grid.
EXEMPT = {
    ("seld_capi.hip", "st.num_cus = prop.multiProcessorCount;"): "where the count comes from",
    ("seld_capi.hip", "if (n < st.num_cus) st.num_cus = static_cast<int>(n);"): "the SELD_CUS limit itself",
    ("seld_capi.hip", "return st ? st->num_cus : kErrNotInitialised;"): "seld_num_cus: reports the count",
    ("seld_common.h", "int num_cus = 0;"): "the field's declaration",
}
