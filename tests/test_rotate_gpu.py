"""GPU tests of the rotation augmentation in azimuth steps (csrc/rotate.hip, seld_augment.py): the
rotation terms against float64, the rotating pair bit-equal to the pair of csrc/augment.hip at quarter turns, the rotated
path against the same formulas in float64, the physics (a rotated recording with shifted metadata, built from scratch) and
the training path.  Input: the plane-wave clips of tests/rotate_ref.py, 50-frame windows with hop 10 on a 150-frame timeline."""
import math

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import rotate_ref
from oracle import features as ofeat

pytestmark = pytest.mark.gpu

WINDOW, HOP = 50, 10
I, J = 18, 36
STARTS = [0, 10, 30, 57, 90, 100, 120, 140]          # B = 8; the last window runs 40 frames past the 150-frame timeline
CONFIG_NAMES = ("FEATURE_SET", "FOA_CHANNEL_ORDER", "AUGMENT_SPATIAL", "AUGMENT_ROTATE", "AUGMENT_TIME_MASKS",
                "AUGMENT_TIME_MASK_MAX", "AUGMENT_FREQ_MASKS", "AUGMENT_FREQ_MASK_MAX", "AUGMENT_MASK_VALUE", "WINDOW_LENGTH",
                "HOP_LENGTH")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


@pytest.fixture
def class_config():
    """Switches are class attributes (config.py is edited in place upstream; dataset.py and trainer.py each hold an instance)."""
    from config import Config
    saved = {k: getattr(Config, k) for k in CONFIG_NAMES}
    yield Config
    for k, v in saved.items():
        setattr(Config, k, v)


def _dataset(Config, dev, feature_set, order, clips=None, rows=None, rotate=True, window=WINDOW, hop=HOP):
    import dataset
    Config.FEATURE_SET, Config.FOA_CHANNEL_ORDER, Config.AUGMENT_ROTATE = feature_set, order, rotate
    Config.WINDOW_LENGTH, Config.HOP_LENGTH = window * 480, hop * 480
    if clips is None:
        clips = [rotate_ref.plane_wave_clip(order, n) for n in range(3)]
        rows = [rotate_ref.clip_rows() for _ in clips]
    ds = dataset.SELDDataset.from_pcm(clips, rows, device=dev)
    Config.AUGMENT_ROTATE = False
    return ds


def _masked_rows(rows, rng, window=WINDOW):
    """Time / frequency masks in the shapes tests/test_augment_gpu.py cycles through, on top of the spatial fields given."""
    for r in range(len(rows)):
        kind = r % 4
        if kind == 0:
            tl, fl = rng.integers(0, 15, 2), rng.integers(0, 20, 2)
            rows[r, 1:9] = (rng.integers(0, window - tl[0] + 1), tl[0], rng.integers(0, window - tl[1] + 1), tl[1],
                            rng.integers(0, 64 - fl[0] + 1), fl[0], rng.integers(0, 64 - fl[1] + 1), fl[1])
        elif kind == 1:
            rows[r, 1:9] = (10, 0, window - 1, 0, 0, 0, 63, 0)                       # empty
        elif kind == 2:
            rows[r, 1:9] = (0, 20, window - 1, 1, 0, 64, 5, 3)                       # full width in frequency
        else:
            rows[r, 1:9] = (window - 6, 6, window - 2, 2, 64 - 7, 7, 0, 1)          # touching the ends
    return rows


# ------------------------------------------------------------------------------------------ 1. rotation terms

@pytest.mark.parametrize("order", ["WYZX", "WXYZ"])
@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_rotation_terms_match_float64(gpu_device, order, dtype):
    """10 log10 of P_X and P_Y within the log-mel bar of tests/logmel_checks.py (1e-4 dB on elements within 40 dB of the
    frame peak); |C - C_ref| <= 2.3e-5 sqrt(P_X P_Y) -- the same bar as a relative power -- on the elements where both are."""
    import seld_native
    clips = [rotate_ref.plane_wave_clip(order, n) for n in range(2)]
    if dtype == "int16":
        clips = [ofeat.pcm_to_int16(c) for c in clips]
    pcm = torch.stack(clips).to(gpu_device)
    terms = seld_native.foa_rotation_terms(seld_native.stft(pcm), order)
    assert tuple(terms.shape) == (2, 51, 3, 64) and terms.dtype == torch.float32
    got = terms.cpu().numpy().astype(np.float64)
    one = seld_native.foa_rotation_terms(seld_native.stft(pcm[1]), order)
    assert torch.equal(one, terms[1])
    for n, clip in enumerate(clips):
        ref = rotate_ref.rotation_terms_f64((ofeat.int16_to_pcm(clip) if dtype == "int16" else clip).numpy(), order)   # [3, 64, F]
        g = got[n].transpose(1, 2, 0)
        strong = []
        for c in range(2):
            ref_db = 10.0 * np.log10(np.maximum(ref[c], 1e-10))
            ok = ref_db >= ref_db.max(axis=0, keepdims=True) - 40.0
            err = np.abs(10.0 * np.log10(np.maximum(g[c], 1e-10)) - ref_db)[ok].max()
            print(f"{order} {dtype} clip {n} term {c}: max |dB diff| {err:.3e} over {ok.mean():.3f} of the elements")
            assert err <= 1e-4
            strong.append(ok)
        both = strong[0] & strong[1]
        ratio = (np.abs(g[2] - ref[2]) / (2.3e-5 * np.sqrt(ref[0] * ref[1])))[both].max()
        print(f"{order} {dtype} clip {n} cross term: worst error / bound {ratio:.3f}; max |C| / sqrt(P_X P_Y) "
              f"{(np.abs(ref[2]) / np.sqrt(ref[0] * ref[1]))[both].max():.3f}")
        assert both.mean() > 0.5 and ratio <= 1.0
        assert (ref[2] < 0).any() and (ref[2] > 0).any()


# ------------------------------------------------------------------------------------------ 2. labels, every transform

def test_label_gather_equals_the_restatement_for_every_transform(gpu_device):
    import seld_native
    rng = np.random.default_rng(7)
    total = 150
    mask = np.where(rng.random((total, I * J)) < 0.03, rng.integers(1, 1 << 13, (total, I * J)), 0).astype(np.uint16)
    combos = [(m, s, e) for m in (0, 1) for e in (0, 1) for s in range(J)]
    rows = np.zeros((len(combos), 12), dtype=np.int32)
    starts = []
    for n, (m, s, e) in enumerate(combos):
        k = n % 4                                                     # the total is reached through every split of (k, r)
        rows[n, 0], rows[n, 9] = (m << 3) | (k << 1) | e, (s - 9 * k) % J
        starts.append(STARTS[n % len(STARTS)] if n % 11 else total + 5)             # some windows wholly past the end
    mask_d = torch.from_numpy(mask).to(gpu_device)
    params = seld_native.augment_params(rows, len(rows), WINDOW, gpu_device, steps=J)
    out = torch.from_numpy(np.full((len(rows), WINDOW, I * J), 0xFFFF, dtype=np.uint16)).to(gpu_device)
    got = seld_native.gather_windows_permute_rotate(mask_d, torch.as_tensor(starts), WINDOW, params, I, J, out=out)
    assert got.data_ptr() == out.data_ptr()
    got = got.cpu().numpy()
    for n, (m, s, e) in enumerate(combos):
        want = np.zeros((WINDOW, I * J), dtype=np.uint16)
        live = max(0, min(WINDOW, total - starts[n]))
        want[:live] = rotate_ref.permute_cells(mask[starts[n]:starts[n] + live], m, s, e)
        assert np.array_equal(got[n], want), (m, s, e)
    # a device table is trusted no further than its bits: steps outside 0..J-1 are reduced by a non-negative modulo
    hostile = torch.from_numpy(rows[:8].copy()).to(gpu_device)
    hostile[:, 9] += torch.tensor([-36, 72, -72, 36, 36 * 1000, -36 * 1000, 360, -360], dtype=torch.int32, device=gpu_device)
    again = seld_native.gather_windows_permute_rotate(mask_d, torch.as_tensor(starts[:8]), WINDOW, hostile, I, J)
    assert np.array_equal(again.cpu().numpy(), got[:8])


# ------------------------------------------------------------------------------------------ 3. quarter turns: bit-equal

@pytest.mark.parametrize("channels,order,mask_value,with_out", [(4, "WYZX", 0.0, False), (4, "WXYZ", -80.0, True),
                                                               (7, "WYZX", -80.0, True), (7, "WXYZ", 0.0, False)])
def test_quarter_turn_totals_are_bit_equal_to_the_augmenting_pair(gpu_device, channels, order, mask_value, with_out):
    """Every pattern (m, k, e) reached as (k, r = 0), as (k = 0, r = k J/4) and mixed (k = 1, r = J/4 -> two quarter turns):
    the rotating pair writes the bits of seld_window_gather_augment / seld_window_permute_mask under (m, total k, e).  The
    copy path never reads the rotation terms: they are NaN here."""
    import seld_augment
    import seld_native
    dev = gpu_device
    rng = np.random.default_rng(channels)
    total = 150
    spec = (rng.standard_normal((total, channels, 64)) * 30).astype(np.float32)
    spec[rng.random(spec.shape) < 0.01] = 0.0
    spec[rng.random(spec.shape) < 0.01] = -0.0
    mask = np.where(rng.random((total, I * J)) < 0.03, rng.integers(1, 1 << 13, (total, I * J)), 0).astype(np.uint16)
    rot = torch.full((total, 3, 64), float("nan"), device=dev)
    table = seld_augment.channel_table("logmel" if channels == 4 else "logmel_iv", channels, order)
    cases = []                                                        # (row pattern, r, equivalent pattern)
    for p in range(16):
        m, k, e = seld_augment.decode(p)
        cases.append((p, 0, p))
        cases.append(((m << 3) | e, k * J // 4, p))
    for m, e in ((0, 0), (1, 0), (0, 1), (1, 1)):
        cases.append(((m << 3) | (1 << 1) | e, J // 4, (m << 3) | (2 << 1) | e))    # mixed: k = 1 and r = J/4
        cases.append(((m << 3) | (3 << 1) | e, 3 * J // 4, (m << 3) | (2 << 1) | e))  # 3 + 3 quarter turns wrap to 2
    rows = _masked_rows(np.zeros((len(cases), 12), dtype=np.int32), rng)
    plain = rows.copy()
    for n, (p, r, equivalent) in enumerate(cases):
        rows[n, 0], rows[n, 9], plain[n, 0] = p, r, equivalent
    starts = torch.as_tensor([(STARTS + [total, -20])[n % 10] for n in range(len(cases))])
    spec_d, mask_d = torch.from_numpy(spec).to(dev), torch.from_numpy(mask).to(dev)
    shape = (len(cases), WINDOW, channels, 64)
    out_s = torch.full(shape, float("nan"), device=dev) if with_out else None
    out_m = torch.from_numpy(np.full((len(cases), WINDOW, I * J), 0xFFFF, dtype=np.uint16)).to(dev) if with_out else None
    params = seld_native.augment_params(rows, len(rows), WINDOW, dev, steps=J)
    got_s = seld_native.gather_windows_rotate(spec_d, rot, starts, WINDOW, params, table, order, J, channels, mask_value, out=out_s)
    got_m = seld_native.gather_windows_permute_rotate(mask_d, starts, WINDOW, params, I, J, out=out_m)
    if with_out:
        assert got_s.data_ptr() == out_s.data_ptr() and got_m.data_ptr() == out_m.data_ptr()
    plain_params = seld_native.augment_params(plain, len(plain), WINDOW, dev)
    want_s = seld_native.gather_windows_augment(spec_d, starts, WINDOW, plain_params, table, channels, mask_value)
    want_m = seld_native.gather_windows_permute(mask_d, starts, WINDOW, plain_params, I, J)
    assert torch.equal(got_s.view(torch.int32), want_s.view(torch.int32))
    assert torch.equal(got_m.view(torch.int16), want_m.view(torch.int16))
    assert (want_s == mask_value).any() and want_m.cpu().numpy().any() and not torch.isnan(got_s).any()
    # and the old pair ignores slot [9]
    old_s = seld_native.gather_windows_augment(spec_d, starts, WINDOW, params, table, channels, mask_value)
    zero_step = rows.copy()
    zero_step[:, 9] = 0
    ref_s = seld_native.gather_windows_augment(spec_d, starts, WINDOW, seld_native.augment_params(zero_step, len(rows), WINDOW, dev),
                                               table, channels, mask_value)
    assert torch.equal(old_s.view(torch.int32), ref_s.view(torch.int32))


def test_c_abi_rejects_what_it_does_not_support(gpu_device):
    import seld_augment
    import seld_native
    dev = gpu_device
    params = seld_native.augment_params(np.zeros((1, 12), np.int32), 1, WINDOW, dev)
    starts = torch.zeros(1, dtype=torch.int64)
    rot = torch.zeros((60, 3, 64), device=dev)
    table5 = np.tile(np.arange(5, dtype=np.uint8), (16, 1))
    with pytest.raises(seld_native.SeldNativeError, match="-4"):                    # 5 channels: no rotation defined
        seld_native.gather_windows_rotate(torch.zeros((60, 5, 64), device=dev), rot, starts, WINDOW, params, table5)
    table4 = seld_augment.channel_table("logmel", 4)
    with pytest.raises(seld_native.SeldNativeError, match="-4"):                    # J % 4 != 0
        seld_native.gather_windows_rotate(torch.zeros((60, 4, 64), device=dev), rot, starts, WINDOW, params, table4, J=34)
    with pytest.raises(seld_native.SeldNativeError, match="-4"):                    # J > SELD_ROTATE_MAX_STEPS
        seld_native.gather_windows_rotate(torch.zeros((60, 4, 64), device=dev), rot, starts, WINDOW, params, table4, J=76)
    with pytest.raises(seld_native.SeldNativeError):                                # rot of another length
        seld_native.gather_windows_rotate(torch.zeros((61, 4, 64), device=dev), rot, starts, WINDOW, params, table4)
    with pytest.raises(seld_native.SeldNativeError, match="-4"):
        seld_native.gather_windows_permute_rotate(torch.from_numpy(np.zeros((60, 20 * 34), dtype=np.uint16)).to(dev), starts,
                                                  WINDOW, params, 20, 34)


# ------------------------------------------------------------------------------------------ 4. rotated path vs float64

@pytest.mark.parametrize("feature_set,order,mask_value", [("logmel", "WYZX", 0.0), ("logmel", "WXYZ", -80.0),
                                                          ("logmel_iv", "WYZX", -80.0), ("logmel_iv", "WXYZ", 0.0)])
def test_rotated_windows_match_the_formulas_in_float64(gpu_device, class_config, feature_set, order, mask_value):
    """The same combinations evaluated in float64 from the device's own fp32 timeline and terms.  Copied channels, masked
    elements and zero rows: bit-equal.  Computed log-mel: within 1e-5 dB (power_to_db's documented bound) + 1.1e-6 kappa' dB
    (four fp32 roundings, 4 x 2^-24 x 10 / ln 10; kappa' formed with |C|); an element whose float64 power is below 2e-10 may
    also be the -100 dB floor.  Computed intensity vectors: within 3 x 2^-24 (|c IV_x| + |s IV_y|)."""
    import seld_augment
    import seld_native
    dev = gpu_device
    ds = _dataset(class_config, dev, feature_set, order)
    channels = ds.n_channels
    assert ds.total_frames == 150 and tuple(ds.rot_tm.shape) == (150, 3, 64) and channels == (4 if feature_set == "logmel" else 7)
    rng = np.random.default_rng(channels + len(order))
    steps = [1, 4, 13, 22, 35, 17, 8, 28, 10, 26, 3, 33, 20, 5, 31, 14]
    rows = np.zeros((16, 12), dtype=np.int32)
    for n, s in enumerate(steps):
        m, e, k = n & 1, (n >> 1) & 1, (n >> 2) & 3
        rows[n, 0], rows[n, 9] = (m << 3) | (k << 1) | e, (s - 9 * k) % J           # total s, reached with k quarter turns
    rows = _masked_rows(rows, rng)
    rows[4:8, 1:9] = 0                                                              # four windows without masks
    starts = STARTS + STARTS[::-1]
    table = seld_augment.channel_table(feature_set, channels, order)
    params = seld_native.augment_params(rows, len(rows), WINDOW, dev, steps=J)
    out = torch.full((len(rows), WINDOW, channels, 64), float("nan"), device=dev)
    got = seld_native.gather_windows_rotate(ds.spec_tm, ds.rot_tm, torch.as_tensor(starts), WINDOW, params, table, order, J,
                                            channels, mask_value, out=out).cpu().numpy()
    got_m = seld_native.gather_windows_permute_rotate(ds.mask_tm, torch.as_tensor(starts), WINDOW, params, I, J).cpu().numpy()
    want, tol, computed, floor_ok, want_m, rotated = rotate_ref.gather(
        ds.spec_tm.cpu().numpy(), ds.rot_tm.cpu().numpy(), ds.mask_tm.cpu().numpy(), starts, rows, WINDOW,
        seld_augment.rotation_table(J), order, table, channels, mask_value)
    assert rotated.all() and np.isfinite(got).all()
    assert np.array_equal(got_m, want_m) and want_m.any()
    assert np.array_equal(_bits(got)[~computed], _bits(want.astype(np.float32))[~computed])
    assert (got[~computed] == np.float32(mask_value)).any() and (got[:, :, 0] != 0).any() and not got[7, 10:].any()
    err = np.abs(got.astype(np.float64) - want)
    ok = (err <= tol) | (floor_ok & (got == -100.0))
    mel = np.zeros(computed.shape, dtype=bool)
    mel[:, :, :4] = computed[:, :, :4]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(computed & (tol > 0), err / tol, 0.0)
    print(f"{feature_set} {order}: computed log-mel worst error / bound {ratio[mel].max():.3f} (largest bound {tol[mel].max():.2e} dB), "
          f"intensity worst error / bound {ratio[computed & ~mel].max() if channels == 7 else 0.0:.3f}; "
          f"{int((floor_ok & computed).sum())} elements near the floor")
    assert ok[computed].all(), float(ratio.max())
    assert computed[:, :, 1:4].any() and (channels == 4 or computed[:, :, 4:].any())
    # a window's output depends on (src, rot, starts[b], params[b]) only: the same windows in another batch
    pick = [9, 2, 2, 15]
    sub = seld_native.gather_windows_rotate(ds.spec_tm, ds.rot_tm, torch.as_tensor([starts[i] for i in pick]), WINDOW,
                                            seld_native.augment_params(rows[pick], len(pick), WINDOW, dev, steps=J), table,
                                            order, J, channels, mask_value).cpu().numpy()
    assert np.array_equal(_bits(sub), _bits(got[pick]))


# ------------------------------------------------------------------------------------------ 5. physical consistency

def _windows(timeline, starts, window):
    out = np.zeros((len(starts), window) + timeline.shape[1:])
    for b, s in enumerate(starts):
        n = max(0, min(window, timeline.shape[0] - int(s)))
        out[b, :n] = timeline[int(s):int(s) + n]
    return out


@pytest.mark.parametrize("order", ["WYZX", "WXYZ"])
def test_rotated_windows_equal_the_windows_of_the_rotated_recording(gpu_device, class_config, order):
    """Dataset A: the plane-wave clips, constructed with the switch on, gathered with (m, r, e).  Dataset B: built from
    scratch from the rotated clips (tests/rotate_ref.py, float64 rotation) and the shifted metadata.  Labels and W / Z log-mel
    bit-equal; X' / Y' log-mel within 1e-4 kappa dB of the float64 oracle on the rotated clip, over elements within 40 dB of
    the frame peak with kappa <= 100 (at most 2 % per case are left out for kappa); intensity vectors within 1e-4 of
    foa_intensity_f64 on the rotated clip."""
    dev = gpu_device
    clips = [rotate_ref.plane_wave_clip(order, n) for n in range(3)]
    rows = [rotate_ref.clip_rows() for _ in clips]
    ds_a = _dataset(class_config, dev, "logmel_iv", order, clips, rows)
    idx = [0, 1, 3, 5, 9, 10, 12, 14]
    starts = ds_a.window_starts[idx]
    assert ds_a.total_frames == 150 and len(ds_a) == 15 and ds_a.window_length_frames == WINDOW and starts[-1] == 140
    cx, cy, cz = order.index("X"), order.index("Y"), order.index("Z")
    terms = np.concatenate([rotate_ref.rotation_terms_f64(c.numpy(), order)[:, :, :50].transpose(2, 0, 1) for c in clips])
    plain_s, plain_m = (t.cpu().numpy() for t in ds_a.device_batch(idx))
    worst = worst_iv = most_left_out = 0.0
    for r in (1, 4, 13, 22, 35):
        for m, e in ((0, 0), (1, 0), (0, 1), (1, 1)):
            t_clips = [torch.from_numpy(rotate_ref.pcm_transformed(c.numpy(), m, r, e, order).astype(np.float32)) for c in clips]
            t_rows = [rotate_ref.rows_transformed(x, m, r, e) for x in rows]
            ds_b = _dataset(class_config, dev, "logmel_iv", order, t_clips, t_rows, rotate=False)
            assert ds_b.rot_tm is None
            params = np.zeros((len(idx), 12), dtype=np.int32)
            params[:, 0], params[:, 9] = (m << 3) | e, r
            aug_s, aug_m = (t.cpu().numpy() for t in ds_a.device_batch(idx, augment=params))
            ref_s, ref_m = (t.cpu().numpy() for t in ds_b.device_batch(idx))
            assert np.array_equal(aug_m, ref_m) and ref_m.any() and not np.array_equal(aug_m, plain_m), (m, r, e)
            for c in (0, cz):
                assert np.array_equal(_bits(aug_s[:, :, c]), _bits(ref_s[:, :, c])), (m, r, e, c)
            # float64 oracle on the rotated clips as they were fed (fp32 samples), cropped and concatenated like the timeline
            mel_t = np.concatenate([ofeat.logmel_f64(c.numpy().astype(np.float64), return_mel=True)[1][:, :, :50].transpose(2, 0, 1)
                                    for c in t_clips])                              # [150, 4, 64] linear
            c_, sn = math.cos(rotate_ref.angle(r)), math.sin(rotate_ref.angle(r))
            kx, ky = rotate_ref.cancellation(terms[:, 0], terms[:, 1], np.sqrt(terms[:, 0] * terms[:, 1]), c_, sn,
                                             mel_t[:, cx], mel_t[:, cy])
            for c, kappa in ((cx, kx), (cy, ky)):
                ref_db = 10.0 * np.log10(np.maximum(mel_t[:, c], 1e-10))
                strong = ref_db >= ref_db.max(axis=1, keepdims=True) - 40.0
                keep = strong & (kappa <= 100.0)
                left_out = 1.0 - keep.sum() / strong.sum()
                most_left_out = max(most_left_out, left_out)
                assert left_out <= 0.02, (m, r, e, c, left_out)
                err = np.abs(aug_s[:, :, c].astype(np.float64) - _windows(ref_db, starts, WINDOW))
                ratio = (err / (1e-4 * np.maximum(_windows(kappa, starts, WINDOW), 1.0)))[_windows(keep, starts, WINDOW) > 0].max()
                worst = max(worst, float(ratio))
                assert ratio <= 1.0, (m, r, e, c, float(ratio))
            iv_tm = np.concatenate([ofeat.foa_intensity_f64(c.numpy().astype(np.float64))[:, :, :50].transpose(2, 0, 1)
                                    for c in t_clips])                              # [150, 3, 64]
            iv_err = float(np.abs(aug_s[:, :, 4:] - _windows(iv_tm, starts, WINDOW)).max())
            worst_iv = max(worst_iv, iv_err)
            assert iv_err <= 1e-4, (m, r, e, iv_err)
            assert np.abs(iv_tm).max() > 0.1 and not np.array_equal(_bits(aug_s[:, :, 4:]), _bits(plain_s[:, :, 4:]))
    print(f"order {order}: worst log-mel error / (1e-4 kappa dB) {worst:.3f}; worst intensity error {worst_iv:.3e}; "
          f"largest share left out for kappa > 100: {100 * most_left_out:.2f} %")


# ------------------------------------------------------------------------------------------ 6. training path

def test_feed_dispatch_and_refusals(gpu_device, class_config):
    """device_batch uses the rotating pair when the dataset holds rotation terms and the plain augmenting pair otherwise;
    the feed refuses the switch for a dataset constructed without it and for feature sets without a defined rotation."""
    import dataset
    import seld_augment
    import trainer
    dev = gpu_device
    with_terms = _dataset(class_config, dev, "logmel", "WYZX")
    without = _dataset(class_config, dev, "logmel", "WYZX", rotate=False)
    assert with_terms.rot_tm is not None and without.rot_tm is None
    assert torch.equal(with_terms.spec_tm, without.spec_tm) and torch.equal(with_terms.mask_tm.view(torch.int16), without.mask_tm.view(torch.int16))
    idx = [0, 4, 14]
    rows = seld_augment.identity_rows(3)
    rows[:, 0], rows[:, 9] = (8, 1, 9), (5, 0, 27)
    a_s, a_m = with_terms.device_batch(idx, augment=rows)
    b_s, b_m = without.device_batch(idx, augment=rows)                               # slot [9] ignored
    assert torch.equal(a_s[1].view(torch.int32), b_s[1].view(torch.int32)) and torch.equal(a_m[1].view(torch.int16), b_m[1].view(torch.int16))
    assert not torch.equal(a_s[0], b_s[0]) and not torch.equal(a_m[0].view(torch.int16), b_m[0].view(torch.int16))
    quarter = rows.copy()
    quarter[2] = seld_augment.identity_rows(1)[0]
    quarter[2, 0] = 9 | (3 << 1)                                                     # (m, k = 3, e): the same transform as r = 27
    c_s, c_m = without.device_batch(idx, augment=quarter)
    assert torch.equal(a_s[2].view(torch.int32), c_s[2].view(torch.int32)) and torch.equal(a_m[2].view(torch.int16), c_m[2].view(torch.int16))
    bad = rows.copy()
    bad[0, 9] = J
    with pytest.raises(ValueError, match="azimuth step"):
        with_terms.device_batch(idx, augment=bad)
    class_config.AUGMENT_ROTATE = True
    loader = DataLoader(without, batch_size=2, shuffle=False)
    with pytest.raises(ValueError, match="AUGMENT_ROTATE"):
        trainer.make_feed(loader, dev, 0, 1)
    assert isinstance(trainer.make_feed(DataLoader(with_terms, batch_size=2, shuffle=False), dev, 0, 1), trainer.DeviceFeed)
    class_config.FEATURE_SET = "logmel_gcc"
    with pytest.raises(ValueError, match="AUGMENT_ROTATE"):                          # construction itself refuses the feature set
        dataset.SELDDataset.from_pcm([ofeat.synth_pcm(3, 8, 24000, "noise")], [rotate_ref.clip_rows()], device=dev)


def test_training_with_rotation_is_reproducible_and_evaluation_is_untouched(gpu_device, class_config, tmp_path):
    """Two train_model runs (2 epochs, small CRNN, captured steps, SEED set) with AUGMENT_ROTATE on give identical loss
    histories, which differ from the run with it off; a window's batch differs between epoch 1 and epoch 2; the evaluation
    feed of the same process returns un-rotated windows.  Timeline: plane-wave clips, the project's 250-frame windows."""
    import trainer
    cfg = trainer.config
    names = ("MODEL_TYPE", "CRNN_CNN_CHANNELS", "CRNN_RNN_HIDDEN", "CRNN_DROPOUT", "NUM_EPOCHS", "BATCH_SIZE", "SEED",
             "OUTPUT_PATH", "CHECKPOINT_PATH", "GRAPH_STEP", "DEVICE_FEED")
    saved = {k: getattr(cfg, k) for k in names}
    saved_det = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    shadowed = "FEATURE_SET" in vars(cfg)                 # an earlier test may have left an instance attribute over the class's
    shadow = vars(cfg).get("FEATURE_SET")
    try:
        cfg.FEATURE_SET = "logmel_iv"
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
        cfg.MODEL_TYPE, cfg.CRNN_CNN_CHANNELS, cfg.CRNN_RNN_HIDDEN, cfg.CRNN_DROPOUT = "crnn", [8, 8, 16, 16], 16, 0.0
        cfg.NUM_EPOCHS, cfg.BATCH_SIZE, cfg.SEED, cfg.GRAPH_STEP, cfg.DEVICE_FEED = 2, 4, 11, True, True
        cfg.OUTPUT_PATH, cfg.CHECKPOINT_PATH = tmp_path / "outputs", tmp_path / "checkpoints"
        cfg.OUTPUT_PATH.mkdir()
        cfg.CHECKPOINT_PATH.mkdir()
        clips = [rotate_ref.plane_wave_clip("WYZX", n) for n in range(18)]
        rows = [rotate_ref.clip_rows() for _ in clips]
        train_ds = _dataset(class_config, gpu_device, "logmel_iv", "WYZX", clips[:12], rows[:12], window=250, hop=50)
        test_ds = _dataset(class_config, gpu_device, "logmel_iv", "WYZX", clips[12:], rows[12:], window=250, hop=50)
        assert len(train_ds) == 12 and train_ds.rot_tm is not None
        train_loader = DataLoader(train_ds, batch_size=cfg.BATCH_SIZE, shuffle=True)
        test_loader = DataLoader(test_ds, batch_size=cfg.BATCH_SIZE, shuffle=False)

        def run(on):
            class_config.AUGMENT_ROTATE = on
            assert trainer.graph_step_enabled(gpu_device, 1)
            for old in cfg.CHECKPOINT_PATH.glob("*.pth"):
                old.unlink()
            _, history = trainer.train_model(train_loader=train_loader, test_loader=test_loader, device=gpu_device)
            assert history["total_epochs"] == 2 and history["config"]["batch_source"] == "DeviceFeed"
            return history["train_losses"], history["test_losses"]

        first, second, off = run(True), run(True), run(False)
        print("rotated:", first, "again:", second, "switch off:", off)
        assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all()
        assert first == second
        assert first[0] != off[0]

        class_config.AUGMENT_ROTATE = True
        ordered = DataLoader(train_ds, batch_size=len(train_ds), shuffle=False)
        feed = trainer.make_feed(ordered, gpu_device, 0, 1)
        e1 = [t.clone() for t in next(iter(feed.batches(1, augment=True)))]
        e1_again = [t.clone() for t in next(iter(feed.batches(1, augment=True)))]
        e2 = [t.clone() for t in next(iter(feed.batches(2, augment=True)))]
        assert torch.equal(e1[0].view(torch.int32), e1_again[0].view(torch.int32))
        assert torch.equal(e1[1].view(torch.int16), e1_again[1].view(torch.int16))
        for w in range(len(train_ds)):
            assert not torch.equal(e1[0][w], e2[0][w]), w
        plain = train_ds.device_batch(list(range(len(train_ds))))
        for got in (next(iter(feed.batches(1))), next(iter(feed.batches(0, augment=False)))):
            assert torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32))
            assert torch.equal(got[1].view(torch.int16), plain[1].view(torch.int16))
        small = trainer.make_feed(DataLoader(train_ds, batch_size=5, shuffle=False), gpu_device, 0, 1)
        parts = [s.clone() for s, _ in small.batches(1, augment=True)]
        assert torch.equal(torch.cat(parts).view(torch.int32), e1[0].view(torch.int32))
        results_on = trainer.test_model(test_loader=test_loader, model_path=cfg.CHECKPOINT_PATH / "best_model.pth",
                                        device=gpu_device, num_visualizations=1, save_visualizations=False)
        class_config.AUGMENT_ROTATE = False
        results_off = trainer.test_model(test_loader=test_loader, model_path=cfg.CHECKPOINT_PATH / "best_model.pth",
                                         device=gpu_device, num_visualizations=1, save_visualizations=False)
        assert results_on["test_loss"] == results_off["test_loss"]
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved_det
        for k, v in saved.items():
            setattr(cfg, k, v)
        if shadowed:
            cfg.FEATURE_SET = shadow
        else:
            del cfg.FEATURE_SET
