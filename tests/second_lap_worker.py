"""Body of tests/test_second_lap_gpu.py: a fresh process with SELD_CUS=1 in its environment, so that the library sizes
every CU-capped grid for ONE compute unit and the kernels walk their grid-stride laps at the tiny shapes of
tests/second_lap_cases.py.  Walks the table, judges every case with the reference and the bar of the kernel's own test module
and prints one ``CASE {json}`` line per case: name, ok, the worst error over its bound (<= 1 passes), and for bit-equal
cases the number of differing elements.  Every return code is checked (seld_native raises), the device is synchronised after
each case, and the first error that is not a judgement -- a HIP error, a refused call -- ends the process with a non-zero
status before another case starts.

    SELD_CUS=1 python tests/second_lap_worker.py [case name ...]"""
import ctypes
import json
import sys
import time
import traceback
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
for p in (str(HERE), str(ROOT), str(ROOT / "sound-event-localization-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import second_lap_cases as table  # noqa: E402


class Judge:
    """Collects one case's comparisons: ``worst`` is the largest error / bound seen, ``differing`` the elements of the
    bit-equal comparisons that differ."""

    def __init__(self):
        self.worst, self.differing, self.notes = 0.0, 0, []

    def close(self, what, error, bound):
        ratio = float(error) / float(bound) if bound > 0 else (0.0 if error == 0 else float("inf"))
        if not np.isfinite(ratio):
            ratio = float("inf")
        if ratio > 1.0:
            self.notes.append(f"{what}: error {float(error):.3e} > bound {float(bound):.3e}")
        self.worst = max(self.worst, ratio)

    def equal(self, what, got, want):
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        if got.shape != want.shape or got.dtype != want.dtype:
            self.notes.append(f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}")
            self.differing += max(got.size, want.size)
            return
        view = {4: np.uint32, 8: np.uint64, 2: np.uint16, 1: np.uint8}[got.dtype.itemsize]
        n = int((got.view(view) != want.view(view)).sum())
        if n:
            self.notes.append(f"{what}: {n} of {got.size} elements differ")
        self.differing += n

    def true(self, what, condition):
        if not bool(condition):
            self.notes.append(f"{what}: does not hold")
            self.differing += 1

    @property
    def ok(self):
        return self.worst <= 1.0 and self.differing == 0


def _labels(n, generator):
    """uint16 class masks: 5 % single events, a few second classes in a cell"""
    cls = torch.randint(0, 13, (n,), generator=generator)
    mask = torch.where(torch.rand(n, generator=generator) < 0.05, 1 << cls, torch.zeros_like(cls))
    mask = mask | torch.where(torch.rand(n, generator=generator) < 0.01, 1 << 5, 0)
    return mask.to(torch.uint16)


# ---- class losses -----------------------------------------------------------------------------------------------------

def run_softmax_mse(dev, shape, j):
    import loss as loss_mod
    import seld_native
    n = shape["n_cells"]
    g = torch.Generator().manual_seed(n)
    logits = torch.randn(n, 14, generator=g) * 2
    mask = _labels(n, g)
    dense = loss_mod.mask_to_dense(mask, 14)
    for dtype in (torch.float32, torch.bfloat16):
        lg = logits.to(dtype)
        seen = lg.double().requires_grad_(True)                       # the logits as the kernel sees them, in float64
        sq = (torch.softmax(seen, -1) - dense.double()) ** 2
        (sq.sum() / 2.0).backward()                                   # d/dz of (1/2) sum: what grad_scale = 1 returns
        ref, ref_grad = sq.mean().item(), seen.grad
        tol = 1e-5 if dtype == torch.float32 else 8e-3
        for labels in (mask.to(dev), dense.to(dev)):
            value, none = seld_native.softmax_mse(lg.to(dev), labels)
            value2, grad = seld_native.softmax_mse(lg.to(dev), labels, grad_scale=1.0)
            what = f"{dtype} {labels.dtype}"
            j.true(what + " value-only returns no gradient", none is None and grad.dtype == dtype)
            j.close(what + " value", abs(value.item() - ref), 1e-5 * ref)
            j.close(what + " value with gradient", abs(value2.item() - ref), 1e-5 * ref)
            j.close(what + " gradient", (grad.double().cpu() - ref_grad).abs().max().item(),
                    tol * max(1.0, ref_grad.abs().max().item()))


def run_softmax_ce(dev, shape, j):
    import loss as loss_mod
    import loss_ce_ref
    import seld_native
    n = shape["n_cells"]
    g = torch.Generator().manual_seed(n + 1)
    logits = torch.randn(n, 14, generator=g) * 2
    mask = _labels(n, g)
    weights = torch.rand(14, generator=g) * 1.95 + 0.05
    dense = loss_mod.mask_to_dense(mask, 14)
    for dtype in (torch.float32, torch.bfloat16):
        lg = logits.to(dtype)
        for gamma in shape["gammas"]:
            want, want_grad, want_w = loss_ce_ref.softmax_ce(lg.float().numpy(), mask.numpy(), weights.numpy(), gamma)
            g_max = np.abs(want_grad).max()
            for labels in (mask.to(dev), dense.to(dev)):
                value, none, w_sum = seld_native.softmax_ce(lg.to(dev), labels, weights.to(dev), gamma, return_weight_sum=True)
                value2, grad = seld_native.softmax_ce(lg.to(dev), labels, weights.to(dev), gamma, grad_scale=1.0)
                what = f"{dtype} {labels.dtype} gamma {gamma}"
                j.true(what + " value-only returns no gradient", none is None and grad.dtype == dtype)
                j.true(what + " both kernels give one value", value.item() == value2.item())
                j.close(what + " value", abs(value.item() - want), 1e-5 * want)
                j.close(what + " W", abs(w_sum.item() - want_w), 1e-7 * want_w)
                j.close(what + " gradient", np.abs(grad.float().cpu().numpy().astype(np.float64) - want_grad).max(),
                        (1e-4 if dtype == torch.float32 else 8e-3) * g_max)


def three_term_reference_f64(logits, dense, grid, w):
    """_three_term_reference of tests/test_loss_gpu.py (the reference's own composition through this package's loss.py),
    evaluated in float64 on the host."""
    import loss as loss_mod
    crit = loss_mod.SMRSELDLoss("mse", *w, grid_size=grid)
    lg = logits.detach().cpu().double().clone().requires_grad_(True)
    dense = dense.cpu().double()
    probs = torch.softmax(lg, -1)
    mse = torch.nn.functional.mse_loss(probs, dense)
    aiur = crit.aiur_loss(probs, dense)
    cl = crit.converging_localization_loss(probs, dense)
    total = w[0] * mse + w[1] * aiur + w[2] * cl
    total.backward()
    return torch.stack((total, mse, aiur, cl)).detach(), lg.grad


def run_smr_loss(dev, shape, j):
    import loss as loss_mod
    import seld_native
    w = (1.0, 0.7, 1.3)
    for frames, grid in shape["grids"]:
        cells = grid[0] * grid[1]
        g = torch.Generator().manual_seed(frames * 100 + grid[0])
        base = torch.randn(1, frames, cells, 14, generator=g) * 2
        cls = torch.randint(0, 13, (frames, cells), generator=g).to(torch.int32)
        mask = torch.where(torch.rand(frames, cells, generator=g) < 0.06, torch.ones(1, dtype=torch.int32) << cls,
                           torch.zeros(1, dtype=torch.int32))
        mask = mask | torch.where(torch.rand(frames, cells, generator=g) < 0.01, torch.full((1,), 1 << 5, dtype=torch.int32),
                                  torch.zeros(1, dtype=torch.int32))
        mask[::3] = 0                                                 # every third frame has no events
        mask = mask.to(torch.uint16).unsqueeze(0)
        dense = loss_mod.mask_to_dense(mask, 14)
        for dtype in (torch.float32, torch.bfloat16):
            logits = base.to(dtype)
            ref_terms, ref_grad = three_term_reference_f64(logits, dense, grid, w)
            tol = 1e-4 if dtype == torch.float32 else 8e-3
            for labels in (mask.to(dev), dense.to(dev)):
                terms, none = seld_native.smr_loss(logits.to(dev), labels, grid, *w, want_grad=False)
                terms2, grad = seld_native.smr_loss(logits.to(dev), labels, grid, *w, want_grad=True)
                what = f"{frames} x {grid} {dtype} {labels.dtype}"
                j.true(what + " value-only returns no gradient", none is None and grad.dtype == dtype)
                j.equal(what + " terms of both kernels", terms.cpu().numpy(), terms2.cpu().numpy())
                j.close(what + " terms", (terms.double().cpu() - ref_terms).abs().max().item(),
                        2e-5 * max(1.0, ref_terms.abs().max().item()))
                j.close(what + " gradient", (grad.double().cpu() - ref_grad).abs().max().item(),
                        tol * ref_grad.abs().max().item())


def run_scale_by_scalar(dev, shape, j):
    import seld_native
    g = torch.Generator().manual_seed(8)
    data = torch.randn(shape["n"], generator=g)
    scale = torch.tensor([0.37], dtype=torch.float32)
    for dtype, tol in ((torch.float32, 1e-4), (torch.bfloat16, 1e-2)):
        want = data.to(dtype).double() * scale.double()
        got = seld_native.scale_by_device_scalar_(data.to(dtype).to(dev), scale.to(dev))
        j.close(f"{dtype}", (got.double().cpu() - want).abs().max().item(), tol * want.abs().max().item())


# ---- labels and the plain gathers -------------------------------------------------------------------------------------

def run_expand_labels(dev, shape, j):
    import seld_native
    from oracle import labels as olab
    n = shape["n_cells"]
    rng = np.random.default_rng(n)
    mask = np.where(rng.random(n) < 0.1, rng.integers(1, 1 << 14, n), 0).astype(np.uint16)
    mask[-1] = 1 << 13                                                # the background bit alone, in the last ragged piece
    got = seld_native.expand_labels(torch.from_numpy(mask).to(dev))
    j.equal("dense labels", got.cpu().numpy(), olab.mask_to_dense(mask))


def _starts(rows, window):
    """in range, overlapping, tail-padded, all padding, repeated"""
    return np.asarray([0, rows // 2, rows - window // 2, rows, rows // 2], dtype=np.int64)


def _oracle_gather(src, starts, window):
    """oracle/windows.py make_window_mask per window: rows past the timeline are zeros (its slicing fits any row type)"""
    from oracle import windows as owin
    flat = src.reshape(src.shape[0], -1)
    return np.stack([owin.make_window_mask(flat, int(s), window) for s in starts]).reshape((len(starts), window) + src.shape[1:])


def run_gather_rows(dev, shape, j):
    import seld_native
    rng = np.random.default_rng(5)
    rows, window = shape["rows"], shape["window"]
    mask = np.where(rng.random((rows, shape["row_bytes"] // 2)) < 0.03, rng.integers(1, 1 << 13, (rows, shape["row_bytes"] // 2)),
                    0).astype(np.uint16)
    starts = _starts(rows, window)
    assert len(starts) == shape["B"]
    out = torch.from_numpy(np.full((len(starts), window, mask.shape[1]), 0xFFFF, dtype=np.uint16)).to(dev)
    got = seld_native.gather_windows(torch.from_numpy(mask).to(dev), torch.from_numpy(starts), window, out=out)
    j.equal("uint16 rows", got.cpu().numpy(), _oracle_gather(mask, starts, window))


def run_gather_rows_affine(dev, shape, j):
    import seld_native
    import standardise_ref
    rng = np.random.default_rng(6)
    rows, window, channels = shape["rows"], shape["window"], shape["row_bytes"] // 256
    spec = (rng.standard_normal((rows, channels, 64)) * 30).astype(np.float32)
    spec[spec == 0] = 1.0
    scale = np.ldexp(1.0, -rng.integers(1, 6, (channels, 64))).astype(np.float32)
    shift = (rng.uniform(-3, 3, (channels, 64)) + 10.0 * np.arange(channels)[:, None]).astype(np.float32)
    starts = _starts(rows, window)
    assert len(starts) == shape["B"]
    got = seld_native.gather_windows_affine(torch.from_numpy(spec).to(dev), torch.from_numpy(starts), window,
                                            torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev))
    want = standardise_ref.affine_exact_scale(_oracle_gather(spec, starts, window), scale, shift)
    padded = (starts[:, None] + np.arange(window)[None, :]) >= rows
    want[padded] = 0.0                                                # rows past the timeline are +0.0, not the shift
    j.equal("standardised fp32 rows", got.cpu().numpy(), want)


# ---- window-grid gathers ----------------------------------------------------------------------------------------------

def run_gather_augment(dev, shape, j):
    import augment_ref
    import seld_augment
    from test_augment_gpu import _params, _run, _timeline
    total, channels, window = shape["rows"], shape["channels"], shape["window"]
    spec, mask = _timeline(channels, total, channels)
    rng = np.random.default_rng(100 + channels)
    patterns = [int(p) for p in rng.permutation(16)[:shape["B"]]]
    starts = [total - 40, 17, 391, total, 17]                         # tail-padded, plain, plain, all padding, repeated
    rows = _params(rng, patterns, window)
    table_ = seld_augment.channel_table("logmel_iv", channels, "WYZX")
    got_s, got_m = _run(dev, spec, mask, starts, rows, table_, channels, -80.0, True)
    want_s, want_m = augment_ref.gather(spec, mask, starts, rows, window, table_, channels, -80.0, 18, 36)
    j.equal("features", got_s, want_s)
    j.equal("labels", got_m, want_m)
    j.true("the masks and the labels are there", (want_s == np.float32(-80.0)).any() and want_m.any())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _bounded(j, what, got, want, tol, computed, floor_ok, at_floor):
    """The float64 judgement of tests/test_rotate_gpu.py and tests/test_mix_gpu.py: a computed element is within its bound,
    or, where the float64 value is at the floor, the floor itself."""
    err = np.abs(got.astype(np.float64) - want)
    ok = (err <= tol) | (floor_ok & at_floor)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(computed & (tol > 0) & ~(floor_ok & at_floor), err / tol, 0.0)
    j.true(what + ": computed elements within their bounds or at the floor", ok[computed].all())
    j.close(what + ": worst computed element", float(ratio[computed].max()) if computed.any() else 0.0, 1.0)
    j.true(what + ": there are computed elements", computed.any())


def run_gather_rotate(dev, shape, j):
    import rotate_ref
    import seld_augment
    import seld_native
    from config import Config
    from test_rotate_gpu import CONFIG_NAMES, I, J, STARTS, WINDOW, _dataset, _masked_rows
    assert WINDOW == shape["window"] and 2 * len(STARTS) == shape["B"]
    feature_set, order, mask_value = "logmel_iv", "WYZX", -80.0
    saved = {k: getattr(Config, k) for k in CONFIG_NAMES}
    try:
        ds = _dataset(Config, dev, feature_set, order)
    finally:
        for k, v in saved.items():
            setattr(Config, k, v)
    channels = ds.n_channels
    assert channels == shape["channels"] and ds.total_frames == 150
    rng = np.random.default_rng(channels + len(order))
    steps = [1, 4, 13, 22, 35, 17, 8, 28, 10, 26, 3, 33, 20, 5, 31, 14]
    rows = np.zeros((16, 12), dtype=np.int32)
    for n, s in enumerate(steps):
        m, e, k = n & 1, (n >> 1) & 1, (n >> 2) & 3
        rows[n, 0], rows[n, 9] = (m << 3) | (k << 1) | e, (s - 9 * k) % J
    rows = _masked_rows(rows, rng)
    rows[4:8, 1:9] = 0
    starts = STARTS + STARTS[::-1]
    table_ = seld_augment.channel_table(feature_set, channels, order)
    params = seld_native.augment_params(rows, len(rows), WINDOW, dev, steps=J)
    out = torch.full((len(rows), WINDOW, channels, 64), float("nan"), device=dev)
    got = seld_native.gather_windows_rotate(ds.spec_tm, ds.rot_tm, torch.as_tensor(starts), WINDOW, params, table_, order, J,
                                            channels, mask_value, out=out).cpu().numpy()
    got_m = seld_native.gather_windows_permute_rotate(ds.mask_tm, torch.as_tensor(starts), WINDOW, params, I, J).cpu().numpy()
    want, tol, computed, floor_ok, want_m, rotated = rotate_ref.gather(
        ds.spec_tm.cpu().numpy(), ds.rot_tm.cpu().numpy(), ds.mask_tm.cpu().numpy(), starts, rows, WINDOW,
        seld_augment.rotation_table(J), order, table_, channels, mask_value)
    j.true("every window is rotated and finite", rotated.all() and np.isfinite(got).all())
    j.equal("labels", got_m, want_m)
    j.equal("copied, masked and zero elements", _bits(got)[~computed], _bits(want.astype(np.float32))[~computed])
    _bounded(j, "rotated elements", got, want, tol, computed, floor_ok, got == -100.0)


def run_gather_mic(dev, shape, j):
    import mic_swap_ref
    import seld_augment
    import seld_native
    from test_mic_swap_gpu import MASK_VALUE, SENTINEL_BITS, TOTAL, _affine, _rows, _sentinel, _timeline
    positions = mic_swap_ref.tetrahedron()
    mics, window = len(positions), shape["window"]
    valid = mic_swap_ref.valid_patterns(positions)
    perm = seld_augment.mic_permutations(positions)
    for (kind, channels), affine in zip(shape["kinds"], (True, False)):
        x = _timeline(channels, 100 + channels)
        freq_channels = mics if kind == "gcc" else channels
        scale = shift = scale_d = shift_d = None
        if affine:
            scale, shift, scale_d, shift_d = _affine(channels, 7, dev)
        rows, starts = _rows([valid[1], valid[-1]], True)           # two swaps x the six starts of the module
        assert len(rows) == shape["B"] and x.shape[0] == TOTAL
        params = seld_native.augment_params(rows, len(rows), window, dev)
        out = _sentinel((len(rows), window, channels, 64), dev)
        got = seld_native.gather_windows_mic(torch.from_numpy(x).to(dev), torch.from_numpy(starts), window, params, perm,
                                             "logmel_" + kind, freq_channels, MASK_VALUE, out=out, scale=scale_d, shift=shift_d)
        want, _ = mic_swap_ref.gather(x, None, starts, rows, window, positions, kind, freq_channels, MASK_VALUE, scale, shift)
        got = got.cpu().numpy()
        j.true(kind + ": every element written", not (_bits(got) == SENTINEL_BITS).any())
        j.equal(kind + " windows", got, want.astype(np.float32))


def run_gather_mix(dev, shape, j):
    import mix_ref
    import seld_native
    from test_mix_gpu import I, J, PAIRS, PARTNER_STARTS, STARTS, WINDOW, _affine, _masked_rows, _table, _timeline
    assert WINDOW == shape["window"] and shape["B"] == 2 * len(PAIRS)
    pairs, partner_starts = PAIRS + PAIRS[::-1], PARTNER_STARTS + PARTNER_STARTS[::-1]
    starts = (STARTS + STARTS[::-1]) * 2
    B = shape["B"]
    for (channels, iv), order, mask_value, affine in zip(shape["sets"], ("WXYZ", "WYZX"), (0.0, -80.0), (False, True)):
        rng = np.random.default_rng(10 * channels + affine)
        spec, mask = _timeline(rng, channels, iv)
        table_ = _table(channels, order)
        rows = _masked_rows(np.zeros((B, 12), dtype=np.int32), rng)
        rows[4:8, 1:9] = 0
        rows[:, 0] = [pa for pa, _ in pairs]
        gains = np.asarray([(0.25, 1.0, 4.0)[n % 3] for n in range(B)], dtype=np.float32)
        partners_host = mix_ref.pack_partners(partner_starts, [pb for _, pb in pairs], gains)
        partners = seld_native.mix_partners(partner_starts, [pb for _, pb in pairs], gains, dev)
        j.equal(f"C = {channels}: partner table", partners.cpu().numpy(), partners_host)
        spec_d, mask_d = torch.from_numpy(spec).to(dev), torch.from_numpy(mask).to(dev)
        scale_h = shift_h = scale = shift = None
        if affine:
            scale_h, shift_h, scale, shift = _affine(rng, channels, dev)
        params = seld_native.augment_params(rows, B, WINDOW, dev)
        starts_t = torch.as_tensor(starts)
        out = torch.full((B, WINDOW, channels, 64), float("nan"), device=dev)
        got = seld_native.gather_windows_mix(spec_d, starts_t, WINDOW, params, partners, table_, channels, mask_value, iv, out=out,
                                             scale=scale, shift=shift).cpu().numpy()
        got_m = seld_native.gather_windows_mix_mask(mask_d, starts_t, WINDOW, params, partners, I, J).cpu().numpy()
        want, tol, computed, floor_ok, want_m, mixed = mix_ref.gather(spec, mask, starts, rows, partners_host, WINDOW, table_, iv,
                                                                       channels, mask_value, scale_h, shift_h, I, J)
        what = f"C = {channels}"
        j.true(what + ": finite, every window mixes", np.isfinite(got).all() and mixed.any(axis=1).all())
        j.equal(what + " labels", got_m, want_m)
        if affine:
            floor_value = np.float32(-100.0) * scale_h + shift_h
            at_floor = np.abs(got - floor_value) <= 2.0 ** -22 * np.abs(floor_value)
        else:
            at_floor = got == -100.0
            j.equal(what + " copied and masked elements", _bits(got)[~computed], _bits(want.astype(np.float32))[~computed])
        _bounded(j, what + " mixed elements", got, want, tol, computed, floor_ok, at_floor)


def run_spectral(dev, shape, j):
    import spectral_ref
    from test_spectral_gpu import SETS, TOTAL, _gathered, _masked_rows, _staged, _timeline
    channels, logmel, freq = SETS["logmel_iv"]
    B, window = shape["B"], shape["window"]
    assert channels == shape["channels"]
    rng = np.random.default_rng(2026)
    starts = [int(s) for s in rng.integers(-30, TOTAL - 10, B)]
    x = _gathered(dev, _timeline(rng, channels, logmel), starts, window)
    rows = _masked_rows(np.zeros((B, 12), dtype=np.int32), rng, window)
    shifts = np.asarray([-63, 1, 2, 63, 0, -5, 30, -18][:B])
    cuts = []
    for _ in range(B):
        tl, fl = rng.integers(0, 30, 2), rng.integers(0, 20, 2)
        cuts.append(tuple((int(rng.integers(0, window - tl[n] + 1)), int(tl[n]), int(rng.integers(0, 64 - fl[n] + 1)), int(fl[n]))
                          for n in range(2)))
    spectral = spectral_ref.rows(shifts, rng.integers(0, 2, B), cuts)
    curves = rng.uniform(-12.0, 12.0, (B, 64)).astype(np.float32)
    got = _staged(dev, x, starts, rows, spectral, curves, logmel, freq, -80.0)
    want = spectral_ref.stage(x, starts, TOTAL, rows, spectral, curves, logmel, freq, -80.0)
    j.equal("the staged batch", got, want.astype(np.float32))
    j.true("the stage changes the batch", not np.array_equal(_bits(got), _bits(x)))


# ---- front end --------------------------------------------------------------------------------------------------------

def _clips(shape, seed):
    from oracle import features as ofeat
    return torch.stack([ofeat.synth_pcm(seed + i, shape["C"], shape["L"], "noise") for i in range(shape["N"])])


def _logmel_close(j, what, got, ref, **kw):
    import logmel_checks
    try:
        worst, _ = logmel_checks.assert_logmel_close(got, ref, **kw)
    except AssertionError as e:
        j.close(what + f" ({e})", 1.0, 0.0)
        return
    j.close(what, worst, logmel_checks.TOL_DB)


def run_logmel(dev, shape, j):
    import seld_native
    from oracle import features as ofeat
    pcm = _clips(shape, 50)
    pcm[1, 2] = 0.0                                                   # a silent channel and an all-zero frame, second clip
    pcm[1, :, 4800:6000] = 0.0
    got = seld_native.logmel(pcm.to(dev), layout="cft").cpu().numpy()
    for n in range(shape["N"]):
        _logmel_close(j, f"clip {n}", got[n], ofeat.logmel_torch(pcm[n]).numpy())
    j.true("the all-zero frame and the silent channel are exactly -100 dB", (got[1, :, :, 11] == -100.0).all() and (got[1, 2] == -100.0).all())
    tcf = seld_native.logmel(pcm.to(dev), layout="tcf").cpu().numpy()
    j.equal("time-major layout", tcf, np.ascontiguousarray(got.transpose(0, 3, 1, 2)))
    ints = ofeat.pcm_to_int16(pcm)
    got16 = seld_native.logmel(ints.to(dev), layout="cft").cpu().numpy()
    for n in range(shape["N"]):
        _logmel_close(j, f"int16 clip {n}", got16[n], ofeat.logmel_torch(ofeat.int16_to_pcm(ints[n])).numpy())


def run_stft(dev, shape, j):
    import seld_native
    from oracle import features as ofeat
    pcm = _clips(shape, 60)
    pcm[1, 2] = 0.0
    pcm[1, :, 4800:6000] = 0.0
    got = torch.view_as_real(seld_native.stft(pcm.to(dev))).cpu().numpy()          # [N, C, F, 481, 2]
    for n in range(shape["N"]):
        ref = np.swapaxes(ofeat.stft_f64(pcm[n].numpy()), -1, -2)                  # [C, F, 481] complex
        err = np.abs((got[n, ..., 0] + 1j * got[n, ..., 1]) - ref).max()
        j.close(f"clip {n}", err, 2e-6 * np.abs(ref).max())
    j.true("the all-zero frame and the silent channel: exactly 0 + 0j", not got[1, :, 11].any() and not got[1, 2].any())


def _foa(dev, shape, j, path):
    import os
    import seld_native
    from oracle import features as ofeat
    pcm = _clips(shape, 70)
    pcm[:, 1] = 0.7 * pcm[:, 0] + 0.3 * pcm[:, 1]                    # correlate X with W: non-trivial vectors
    pcm[1, :, 12000:12100] = 0.0                                      # a stretch of digital silence: eps carries it
    os.environ["SELD_FOA"] = path
    try:
        feat = seld_native.spatial_features(pcm.to(dev), "logmel_iv").cpu()        # [N, F, 7, 64]
    finally:
        del os.environ["SELD_FOA"]
    for n in range(shape["N"]):
        _logmel_close(j, f"{path} clip {n} log-mel", feat[n, :, :4].permute(1, 2, 0).numpy(), ofeat.logmel_torch(pcm[n]).numpy())
        ref = ofeat.foa_intensity_f64(pcm[n].numpy())                              # [3, 64, F]
        j.close(f"{path} clip {n} intensity vectors", np.abs(feat[n, :, 4:].permute(1, 2, 0).numpy() - ref).max(), 1e-4)
        j.true(f"{path} clip {n}: the planted correlation shows", np.abs(ref[0]).max() > 0.1)


def run_logmel_iv(dev, shape, j):
    _foa(dev, shape, j, "fused")


def run_foa_iv(dev, shape, j):
    _foa(dev, shape, j, "spectra")


def run_gcc_phat(dev, shape, j):
    import os
    import seld_native
    from oracle import features as ofeat
    pulse = np.zeros(64)
    pulse[32] = 1.0
    for channels, kernels in ((shape["C"], ("mfma", "planar", "spectra", "fft")), (7, ("mfma",))):    # 7: the two-tile kernel
        pcm = _clips(dict(shape, C=channels), 80 + channels)
        pcm[:, 1, 7:] = pcm[:, 0, :-7].clone()                        # channel 1 = channel 0 delayed by 7 samples
        pcm[1, 2] = 0.0                                               # second clip: a dead microphone ...
        pcm[1, :, 4800:6000] = 0.0                                    # ... and frame 11 all-zero in every channel
        refs = [ofeat.gcc_phat_f64(pcm[n].numpy()) for n in range(shape["N"])]     # [pairs, 64, F]
        pair_list = [(a, b) for a in range(channels) for b in range(a + 1, channels)]
        dead = [p for p, (a, b) in enumerate(pair_list) if 2 in (a, b)]
        for kernel in kernels:
            os.environ["SELD_GCC"] = kernel
            try:
                feat = seld_native.spatial_features(pcm.to(dev), "logmel_gcc").cpu()
            finally:
                del os.environ["SELD_GCC"]
            what = f"C = {channels} {kernel}"
            for n in range(shape["N"]):
                _logmel_close(j, f"{what} clip {n} log-mel", feat[n, :, :channels].permute(1, 2, 0).numpy(),
                              ofeat.logmel_torch(pcm[n]).numpy())
                got = feat[n, :, channels:].permute(1, 2, 0).numpy()
                j.close(f"{what} clip {n}", np.abs(got - refs[n]).max(), 1e-4)
                if n != 1:
                    j.true(f"{what} clip {n}: the planted delay is the peak", (got[0, :, 3:-3].argmax(axis=0) == 39).all())
            got = feat[1, :, channels:].permute(1, 2, 0).numpy()
            j.close(what + ": pairs with the dead microphone are the unit pulse", np.abs(got[dead] - pulse[None, :, None]).max(), 2e-5)
            j.close(what + ": every pair of the all-zero frame is the unit pulse", np.abs(got[:, :, 11] - pulse[None, :]).max(), 2e-5)
            j.true(what + ": the all-zero frame is exactly -100 dB", (feat[1, 11, :channels] == -100.0).all())


def run_nipd(dev, shape, j):
    import nipd_ref
    import seld_native
    from test_nipd_gpu import SENTINEL, SPEED, _phasor_pass
    pcm = _clips(shape, 300)
    pcm[1, 2] = 0.0
    n, channels, frames = shape["N"], shape["C"], table.frames_of(shape["L"])
    _, words = _phasor_pass(pcm.to(dev))
    fb = nipd_ref.library_filterbank()
    for lo, hi in ((50.0, 2000.0), (25.0, 12000.0)):
        _, dev_table = seld_native.nipd_table(dev, lo, hi, SPEED)
        out = torch.full((n, frames, channels - 1, 64), SENTINEL, dtype=torch.float32, device=dev)
        seld_native.nipd_q15(words, out, dev_table)
        got = out.cpu().numpy().astype(np.float64)
        weights = nipd_ref.dense_weights(fb, lo, hi, SPEED)
        host = words.cpu().numpy()
        for i in range(n):
            want = nipd_ref.nipd_from_words(host[i], weights)          # [C - 1, F, 64]
            j.close(f"({lo:g}, {hi:g}) clip {i}", np.abs(got[i].transpose(1, 0, 2) - want).max(), 1e-5)
        empty = ~weights.any(axis=0)
        j.true(f"({lo:g}, {hi:g}): empty bands 0, every element written", (got[..., empty] == 0.0).all() and not (got == SENTINEL).any())
        j.true(f"({lo:g}, {hi:g}): the dead microphone's channel is exactly 0", (got[1, :, 1] == 0.0).all())


def run_rotation_terms(dev, shape, j):
    import rotate_ref
    import seld_native
    order = "WYZX"
    clips = [rotate_ref.plane_wave_clip(order, n) for n in range(shape["N"])]
    assert clips[0].shape[1] == shape["L"]
    pcm = torch.stack(clips).to(dev)
    terms = seld_native.foa_rotation_terms(seld_native.stft(pcm), order)
    got = terms.cpu().numpy().astype(np.float64)
    for n, clip in enumerate(clips):
        ref = rotate_ref.rotation_terms_f64(clip.numpy(), order)                  # [3, 64, F]
        g = got[n].transpose(1, 2, 0)
        strong = []
        for c in range(2):
            ref_db = 10.0 * np.log10(np.maximum(ref[c], 1e-10))
            ok = ref_db >= ref_db.max(axis=0, keepdims=True) - 40.0
            j.close(f"clip {n} power {c}", np.abs(10.0 * np.log10(np.maximum(g[c], 1e-10)) - ref_db)[ok].max(), 1e-4)
            strong.append(ok)
        both = strong[0] & strong[1]
        j.close(f"clip {n} cross term", (np.abs(g[2] - ref[2]) / (2.3e-5 * np.sqrt(ref[0] * ref[1])))[both].max(), 1.0)
        j.true(f"clip {n}: half the elements are strong", both.mean() > 0.5)


# ---- encoder ----------------------------------------------------------------------------------------------------------

def _ratios(j, what, ratios):
    for k, v in ratios.items():
        j.close(f"{what} {k}", v if v == v else float("inf"), 1.0)


def run_conv_tail(dev, shape, j):
    import tail_checks
    from test_tail_parity_gpu import _run
    for mode, c, dtype in shape["cases"]:
        rows, _ = table.tail_rows(mode, c, 1)
        case = tail_checks.make_case(mode, {"bf16": torch.bfloat16, "fp32": torch.float32}[dtype], rows=rows, c=c, integer=False, seed=5)
        _ratios(j, f"mode {mode} C = {c} {dtype}", tail_checks.run_checks(case, _run(case, mode, dev), mode, exact_stats=False))


def run_convfirst(dev, shape, j):
    import convfirst_checks
    from test_convfirst_parity_gpu import _run
    for s in shape["shapes"]:
        geom = convfirst_checks.geometry(s, 1)
        assert geom["groups"] == 2 and geom["per_group"] >= 3, geom
        for family in ("integer", "dyadic"):
            case = convfirst_checks.make_case(family, s)
            dw = torch.empty(64, 4, 3, 3, dtype=torch.float32, device=dev) if s[2] == 64 else None
            ratios = convfirst_checks.run_checks(case, _run(case, dev, dw=dw), 1)
            _ratios(j, f"{family} {s}", ratios)
            j.true(f"{family} {s}: y and dbeta bit-equal", ratios["y"] == 0.0 and ratios["dbeta"] == 0.0)


def run_conv3x3_wgrad(dev, shape, j):
    import seld_native
    from test_conv_wgrad_gpu import _case, _dw
    args = ((1, 1), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False))
    for b, cin, cout, t, f in shape["shapes"]:
        x, dy = _case(b, cin, cout, t, f, dev, seed=b * 1000 + cin + f)
        assert seld_native.conv3x3_wgrad_applicable(x, dy, _dw(cout, cin, torch.bfloat16, dev))
        x64, dy64 = x.cpu().double().contiguous(), dy.cpu().double().contiguous()
        w = torch.empty(cout, cin, 3, 3, dtype=torch.float64)
        ref = torch.ops.aten.convolution_backward(dy64, x64, w, None, *args)[1]
        mag = torch.ops.aten.convolution_backward(dy64.abs(), x64.abs(), w, None, *args)[1]
        for dtype, rounding in ((torch.float32, 0.0), (torch.bfloat16, 2.0 ** -8)):
            dw = seld_native.conv3x3_wgrad(x, dy, _dw(cout, cin, dtype, dev))
            torch.cuda.synchronize()
            err = (dw.double().cpu() - ref).abs()
            j.close(f"{(b, cin, cout, t, f)} {dtype}", (err / (1e-5 * mag + rounding * ref.abs() + 1e-30)).max().item(), 1.0)


# ---- timeline passes --------------------------------------------------------------------------------------------------

def run_balance(dev, shape, j):
    import balance_ref
    import seld_native
    from test_balance_gpu import CELLS, COUNT_SENTINEL, PAD, ROW_SENTINEL, _masks
    seld_native.ensure_init(dev)
    lib, stream = seld_native.load_library(), seld_native._stream_ptr(dev)
    total, window, hop, n_windows = shape["rows"], shape["window"], shape["hop"], shape["n_windows"]
    assert n_windows == (total + hop - 1) // hop
    masks = _masks(total)
    for name in ("random sparse", "cells 512..647", "bit 13"):
        mask = masks[name]
        want_rows = balance_ref.frame_class_mask(mask)
        mask_d = torch.from_numpy(mask).to(dev)
        rows_d = torch.full((total + PAD,), ROW_SENTINEL, dtype=torch.uint16, device=dev)
        seld_native.check(lib.seld_frame_class_mask(ctypes.c_void_p(mask_d.data_ptr()), total, CELLS,
                                                    ctypes.c_void_p(rows_d.data_ptr()), stream), "seld_frame_class_mask")
        got = rows_d.cpu().numpy()
        j.equal(name + ": frame words", got[:total], want_rows)
        j.true(name + ": nothing behind the frame words", (got[total:] == ROW_SENTINEL).all())
        counts_d = torch.full((n_windows + PAD, 16), COUNT_SENTINEL, dtype=torch.int32, device=dev)
        seld_native.check(lib.seld_window_class_frames(ctypes.c_void_p(rows_d.data_ptr()), total, window, hop, n_windows, 14,
                                                       ctypes.c_void_p(counts_d.data_ptr()), stream), "seld_window_class_frames")
        got_counts = counts_d.cpu().numpy()
        j.equal(name + ": window counts", got_counts[:n_windows], balance_ref.window_class_frames(want_rows, window, hop, n_windows, 14))
        j.true(name + ": nothing behind the counts", (got_counts[n_windows:] == COUNT_SENTINEL).all())


def run_feature_moments(dev, shape, j):
    import seld_native
    import standardise_ref
    x = standardise_ref.feature_like(shape["rows"] + shape["channels"], shape["rows"], shape["channels"])
    got = seld_native.feature_moments(torch.from_numpy(x).to(dev))
    j.equal("moments", got.cpu().numpy(), standardise_ref.moments(x))


def run_pcen(dev, shape, j):
    import pcen_ref
    import seld_native
    N, T, c_log, c_total = shape["N"], shape["T"], shape["C_log"], shape["C_total"]
    x = pcen_ref.inputs(100 + T, N, T, c_log, c_total)
    x_d = torch.from_numpy(x).to(dev)
    for setting in (0, 3):
        tau, alpha, delta, r, eps = pcen_ref.SETTINGS[setting]
        want = pcen_ref.ref64(x, c_log, np.float32(pcen_ref.coefficient(tau)), alpha, delta, r, eps)
        y = seld_native.pcen(x_d, c_log, seld_native.pcen_coefficient(tau), alpha, delta, r, eps)
        k = pcen_ref.error_factor(y[:, :, :c_log].cpu().numpy(), want, delta, r)
        j.close(f"setting {setting}: error factor", k, pcen_ref.DEVICE_FACTOR * pcen_ref.REF32_K[setting])
        j.equal(f"setting {setting}: the other channels", y[:, :, c_log:].cpu().numpy(), x[:, :, c_log:])
        again = x_d.clone()
        seld_native.pcen(again, c_log, seld_native.pcen_coefficient(tau), alpha, delta, r, eps, out=again)
        j.equal(f"setting {setting}: in place", again.cpu().numpy(), y.cpu().numpy())


RUNNERS = {name[4:]: fn for name, fn in list(globals().items()) if name.startswith("run_")}


def main(argv):
    import seld_native
    assert torch.cuda.is_available(), "the second-lap worker needs a GPU"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cus = seld_native.num_cus(dev)
    print(f"WORKER num_cus {cus}", flush=True)
    assert cus == 1, f"SELD_CUS=1 did not take effect: the library sees {cus} compute units"
    wanted = set(argv) or {c.name for c in table.CASES}
    started = time.perf_counter()
    for case in table.CASES:
        if case.name not in wanted:
            continue
        for launch in case.launches(case.shape, cus):                 # what this process really walks
            assert table.laps(launch) >= 3 and table.ragged(launch), (case.name, launch)
        j = Judge()
        t0 = time.perf_counter()
        try:
            RUNNERS[case.name](dev, case.shape, j)
            torch.cuda.synchronize(dev)
        except BaseException:                                         # a HIP error, a refused call: nothing runs after it
            traceback.print_exc()
            print("FATAL " + json.dumps({"name": case.name}), flush=True)
            return 3
        print("CASE " + json.dumps({"name": case.name, "ok": j.ok, "worst": j.worst, "differing": j.differing,
                                    "bit_equal": case.bit_equal, "seconds": round(time.perf_counter() - t0, 3),
                                    "notes": j.notes[:6]}), flush=True)
    print(f"WORKER seconds {time.perf_counter() - started:.2f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
