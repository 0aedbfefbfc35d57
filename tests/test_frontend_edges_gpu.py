"""GPU parity tests of the audio front end (csrc/logmel.hip, spatial.hip, nipd.hip) on the input families of
tests/frontend_cases.py: digital silence next to loud frames in every slot of the two-frame packing, on both load paths
and at both clip ends; silent and sounding channels in one frame; full-scale int16; power-of-two scaled copies.  What a
frame is held to, the fp32-peer rule for tonal frames and the Q15 bounds: tests/frontend_checks.py (the same checks run
on the lane emulator's outputs in tests/test_frontend_cases_cpu.py).  Clips have at most 18 frames; every case is a few
launches.  Each test prints the worst figure per family (kernel error, fp32 peer error, tolerance): DESIGN.md 7.5 quotes them.
"""
import numpy as np
import pytest
import torch

import frontend_cases as fc
import frontend_checks as chk

pytestmark = pytest.mark.gpu

GUARD = 4096                                         # sentinel elements either side of a guarded buffer


def _dev(x, device):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def _batch(case):
    """[3, C, L]: the clip, its channels rotated by one, its channels reversed -- same length, same all-zero frames in
    other channels."""
    x = case.pcm
    return np.stack([x, np.roll(x, 1, axis=0), x[::-1]])


def _worst(table, name, figures):
    row = table.setdefault(name, {})
    for k, v in figures.items():
        row[k] = max(row.get(k, 0.0), v)


def _report(what, table):
    for name, row in table.items():
        print(f"{what} {name}: " + " ".join(f"{k}={v:.3e}" for k, v in row.items()))


def _families(channels, f32_only=False):
    out = [(fc.loud_gap, c) for c in fc.loud_gap(channels)] + [(fc.loud_gap_one_channel, c) for c in fc.loud_gap_one_channel(channels)]
    out += [(fc.scaled, c) for c in fc.scaled(channels)]
    if not f32_only:
        out += [(fc.full_scale_i16, c) for c in fc.full_scale_i16(channels)]
    return out


def _guarded(shape, dtype, device, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=device)
    return buf[GUARD:GUARD + n].view(shape), buf


def _guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


# ---------------------------------------------------------------------------------------------------- STFT

@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_stft(gpu_device, dtype):
    import seld_native
    table = {}
    cases = _families(4, f32_only=True) if dtype == "float32" else [(fc.full_scale_i16, c) for c in fc.full_scale_i16(4)]
    for family, case in cases:
        r = chk.ref_of(case, family)
        got = seld_native.stft(_dev(case.pcm, gpu_device))                         # [C, F, 481]
        _worst(table, case.family, chk.check_stft(r, got.cpu().numpy()))
        if dtype == "int16":                                                       # the same samples through the f32 entry point
            chk.check_stft(r, seld_native.stft(_dev(fc.as_float(case), gpu_device)).cpu().numpy())
        batch = _dev(_batch(case), gpu_device)
        both = seld_native.stft(batch)
        assert torch.equal(torch.view_as_real(both[0]), torch.view_as_real(got))
        for i in (1, 2):
            assert torch.equal(torch.view_as_real(both[i]), torch.view_as_real(seld_native.stft(batch[i]))), (case.name, i)
    _report("stft", table)


# ---------------------------------------------------------------------------------------------------- log-mel

@pytest.mark.parametrize("layout", ["cft", "tcf"])
def test_logmel(gpu_device, layout):
    import seld_native
    table = {}
    for family, case in _families(4):
        r = chk.ref_of(case, family)
        got = seld_native.logmel(_dev(case.pcm, gpu_device), layout=layout)
        cft = got if layout == "cft" else got.permute(1, 2, 0)
        _worst(table, case.family, chk.check_logmel(r, cft.cpu().numpy()))
        if case.pcm.dtype == np.int16:
            # the same samples through the f32 entry point: the bar of tests/test_logmel_gpu.py test_golden_int16_vector
            got_f = seld_native.logmel(_dev(fc.as_float(case), gpu_device), layout=layout)
            chk.check_logmel(r, (got_f if layout == "cft" else got_f.permute(1, 2, 0)).cpu().numpy())
            assert (got - got_f).abs().max().item() <= 2e-5
        batch = _dev(_batch(case), gpu_device)
        both = seld_native.logmel(batch, layout=layout)
        assert torch.equal(both[0], got)
        for i in (1, 2):
            assert torch.equal(both[i], seld_native.logmel(batch[i], layout=layout)), (case.name, i)
    _report(f"logmel {layout}", table)


# ---------------------------------------------------------------------------------------------------- GCC-PHAT

@pytest.mark.parametrize("kernel", ["mfma", "planar", "spectra", "fft"])
@pytest.mark.parametrize("channels", [2, 4, 6, 7, 8])
def test_gcc_phat(gpu_device, channels, kernel, monkeypatch):
    """6 and 7 channels = 15 and 21 pairs, either side of the 16-pair tile; 6 runs the one-channel family only."""
    import seld_native
    monkeypatch.setenv("SELD_GCC", kernel)
    table = {}
    cases = [(fc.loud_gap_one_channel, c) for c in fc.loud_gap_one_channel(6)] if channels == 6 else _families(channels)
    for family, case in cases:
        r = chk.ref_of(case, family)
        pcm = _dev(case.pcm, gpu_device)
        feat = seld_native.spatial_features(pcm, "logmel_gcc")                     # [F, C + pairs, 64]
        assert tuple(feat.shape) == (r.frames, channels + channels * (channels - 1) // 2, 64)
        host = feat.cpu().numpy()
        chk.check_logmel(r, host[:, :channels].transpose(1, 2, 0))
        figures = chk.check_gcc(r, host[:, channels:].transpose(1, 2, 0), q15=kernel in ("mfma", "planar"))
        _worst(table, case.family, figures)
        if case.frames in (6, 18):                                                 # batched N = 3: bit-equal to per-clip runs
            batch = _dev(_batch(case), gpu_device)
            both = seld_native.spatial_features(batch, "logmel_gcc")
            assert torch.equal(both[0], feat)
            for i in (1, 2):
                assert torch.equal(both[i], seld_native.spatial_features(batch[i], "logmel_gcc")), (case.name, i)
    _report(f"gcc {kernel} C={channels}", table)


# ---------------------------------------------------------------------------------------------------- FOA intensity

@pytest.mark.parametrize("path", ["fused", "spectra"])
def test_foa_intensity(gpu_device, path, monkeypatch):
    import seld_native
    monkeypatch.setenv("SELD_FOA", path)
    table = {}
    for family, case in _families(4):
        r = chk.ref_of(case, family)
        feat = seld_native.spatial_features(_dev(case.pcm, gpu_device), "logmel_iv")       # [F, 7, 64]
        assert tuple(feat.shape) == (r.frames, 7, 64)
        host = feat.cpu().numpy()
        chk.check_logmel(r, host[:, :4].transpose(1, 2, 0))
        _worst(table, case.family, chk.check_iv(r, host[:, 4:].transpose(1, 2, 0)))
        if case.frames in (6, 18):
            batch = _dev(_batch(case), gpu_device)
            both = seld_native.spatial_features(batch, "logmel_iv")
            assert torch.equal(both[0], feat)
            for i in (1, 2):
                assert torch.equal(both[i], seld_native.spatial_features(batch[i], "logmel_iv")), (case.name, i)
    _report(f"foa {path}", table)


# ---------------------------------------------------------------------------------------------------- NIPD

@pytest.mark.parametrize("channels", [2, 4, 6, 7, 8])
def test_nipd(gpu_device, channels):
    import seld_native
    table = {}
    cases = [(fc.loud_gap_one_channel, c) for c in fc.loud_gap_one_channel(6)] if channels == 6 else _families(channels)
    kw = dict(nipd_min_hz=chk.NIPD_LO, nipd_max_hz=chk.NIPD_HI, sound_speed=chk.SPEED)
    for family, case in cases:
        r = chk.ref_of(case, family)
        feat = seld_native.spatial_features(_dev(case.pcm, gpu_device), "logmel_nipd", **kw)        # [F, 2C - 1, 64]
        assert tuple(feat.shape) == (r.frames, 2 * channels - 1, 64)
        host = feat.cpu().numpy()
        chk.check_logmel(r, host[:, :channels].transpose(1, 2, 0))
        _worst(table, case.family, chk.check_nipd(r, host[:, channels:].transpose(1, 0, 2)))
        if case.frames in (6, 18):
            batch = _dev(_batch(case), gpu_device)
            both = seld_native.spatial_features(batch, "logmel_nipd", **kw)
            assert torch.equal(both[0], feat)
            for i in (1, 2):
                assert torch.equal(both[i], seld_native.spatial_features(batch[i], "logmel_nipd", **kw)), (case.name, i)
    _report(f"nipd C={channels}", table)


# ---------------------------------------------------------------------------------------------------- scaled copies

def _phasor_pass(pcm, words_fill=-1, guarded=False):
    """seld_logmel_phasors_* on pcm [N, C, L] (device) into sentinel-filled buffers: (log-mel [N, F, C, 64], words int32
    [N, C, F, pitch], the two whole buffers)."""
    import seld_native
    lib = seld_native.load_library()
    n, c, length = pcm.shape
    index = seld_native.ensure_init(pcm.device)
    frames = seld_native.num_frames(length)
    out, out_buf = _guarded((n, frames, c, 64), torch.float32, pcm.device, chk.SENTINEL)
    words, words_buf = _guarded((n, c, frames, int(lib.seld_phasor_pitch())), torch.int32, pcm.device, words_fill)
    fn = lib.seld_logmel_phasors_f32 if pcm.dtype == torch.float32 else lib.seld_logmel_phasors_i16
    with torch.cuda.device(index):
        seld_native.check(fn(seld_native._p(pcm), n, c, length, seld_native._p(out), frames * c * 64, 64, 1, c * 64,
                             seld_native._p(words), seld_native._stream_ptr(pcm.device)), "seld_logmel_phasors")
    return out, words, out_buf, words_buf


@pytest.mark.parametrize("channels", [4, 7])
def test_scaled_copies(gpu_device, channels, monkeypatch):
    """x and 2^-k x, k = 4, 10: power-of-two scaling is exact in fp32 and the reciprocal square root of a power scaled by
    2^-2k is the exact scaling, so the Q15 words, and GCC-PHAT and NIPD computed from them, are bit-equal; log-mel differs
    by 20 k log10(2) dB to the 2e-5 of tests/test_logmel_gpu.py (the logarithm's rounding).  Intensity carries eps and is
    compared with the oracle only (test_foa_intensity)."""
    import seld_native
    cases = fc.scaled(channels)
    kw = dict(nipd_min_hz=chk.NIPD_LO, nipd_max_hz=chk.NIPD_HI, sound_speed=chk.SPEED)
    for base in (c for c in cases if c.scale_log2 == 0):
        dead = torch.from_numpy(fc.dead_frames(base.pcm).all(axis=0))
        x0 = _dev(base.pcm, gpu_device)
        db0, words0, _, _ = _phasor_pass(x0[None])
        nipd0 = seld_native.spatial_features(x0, "logmel_nipd", **kw)
        gcc0 = {}
        for kernel in ("mfma", "planar"):
            monkeypatch.setenv("SELD_GCC", kernel)
            gcc0[kernel] = seld_native.spatial_features(x0, "logmel_gcc")
        for c in cases:
            if c.pcm.shape != base.pcm.shape or not c.scale_log2:
                continue
            x = _dev(c.pcm, gpu_device)
            db, words, _, _ = _phasor_pass(x[None])
            assert torch.equal(words, words0), c.name
            shift = 20.0 * c.scale_log2 * np.log10(2.0)
            assert (db0 - db - shift)[:, ~dead].abs().max().item() <= 2e-5, c.name
            assert (db[:, dead] == -100.0).all() and (db0[:, dead] == -100.0).all()
            nipd = seld_native.spatial_features(x, "logmel_nipd", **kw)
            assert torch.equal(nipd[:, channels:], nipd0[:, channels:]), c.name
            for kernel in ("mfma", "planar"):
                monkeypatch.setenv("SELD_GCC", kernel)
                gcc = seld_native.spatial_features(x, "logmel_gcc")
                assert torch.equal(gcc[:, channels:], gcc0[kernel][:, channels:]), (c.name, kernel)


# ---------------------------------------------------------------------------------------------------- canaries

@pytest.mark.parametrize("n_clips", [1, 3])
def test_nothing_is_stored_outside_the_outputs(gpu_device, n_clips):
    """Every pass of csrc/logmel.hip into buffers pre-filled with a sentinel, with guards either side: with F % 4 != 0 the
    last iteration is partial, and a store past frame F - 1 would land in the next clip's first frame or in the guard.
    Inside, nothing keeps the sentinel but the seven padding words of a phasor row; the values are those of the public calls."""
    import seld_native
    lib = seld_native.load_library()
    for case in fc.loud_gap(4) + fc.full_scale_i16(4):
        x = _batch(case)[:n_clips]
        pcm = _dev(x, gpu_device)
        n, c, length = pcm.shape
        frames = case.frames
        suffix = "f32" if pcm.dtype == torch.float32 else "i16"
        stream = seld_native._stream_ptr(gpu_device)
        index = seld_native.ensure_init(pcm.device)
        # log-mel, both layouts
        for layout, shape in (("cft", (n, c, 64, frames)), ("tcf", (n, frames, c, 64))):
            out, buf = _guarded(shape, torch.float32, gpu_device, chk.SENTINEL)
            seld_native.logmel(pcm, layout=layout, out=out)
            assert _guards_intact(buf, chk.SENTINEL) and not (out == chk.SENTINEL).any(), (case.name, layout)
            assert torch.equal(out, seld_native.logmel(pcm, layout=layout))
        plain = seld_native.logmel(pcm, layout="tcf")
        # the strided entry point, placing the channels in a wider feature tensor: the other channels keep the sentinel
        wide, buf = _guarded((n, frames, c + 3, 64), torch.float32, gpu_device, chk.SENTINEL)
        with torch.cuda.device(index):
            seld_native.check(getattr(lib, f"seld_logmel_{suffix}_strided")(
                seld_native._p(pcm), n, c, length, seld_native._p(wide), frames * (c + 3) * 64, 64, 1, (c + 3) * 64, stream),
                "seld_logmel_strided")
        assert _guards_intact(buf, chk.SENTINEL) and torch.equal(wide[:, :, :c], plain) and (wide[:, :, c:] == chk.SENTINEL).all()
        # STFT export
        spec, buf = _guarded((n, c, frames, 481, 2), torch.float32, gpu_device, chk.SENTINEL)
        with torch.cuda.device(index):
            seld_native.check(getattr(lib, f"seld_stft_{suffix}")(seld_native._p(pcm), n, c, length, seld_native._p(spec), stream), "seld_stft")
        assert _guards_intact(buf, chk.SENTINEL) and not (spec == chk.SENTINEL).any(), case.name
        assert torch.equal(spec, torch.view_as_real(seld_native.stft(pcm)))
        # phasor pass
        out, words, out_buf, words_buf = _phasor_pass(pcm)
        assert _guards_intact(out_buf, chk.SENTINEL) and _guards_intact(words_buf, -1), case.name
        assert torch.equal(out, plain) and (words[..., 481:] == -1).all()
        host_words = words.cpu().numpy()
        for i in range(n):
            dead = fc.dead_frames(x[i])
            assert not host_words[i][dead][:, :481].any() and host_words[i][~dead][:, :481].any(axis=1).all(), (case.name, i)
        # spectrum pass
        out, out_buf = _guarded((n, frames, c, 64), torch.float32, gpu_device, chk.SENTINEL)
        spec2, buf = _guarded((n, c, frames, 481, 2), torch.float32, gpu_device, chk.SENTINEL)
        with torch.cuda.device(index):
            seld_native.check(getattr(lib, f"seld_logmel_spectrum_{suffix}")(
                seld_native._p(pcm), n, c, length, seld_native._p(out), frames * c * 64, 64, 1, c * 64, seld_native._p(spec2), stream),
                "seld_logmel_spectrum")
        assert _guards_intact(out_buf, chk.SENTINEL) and _guards_intact(buf, chk.SENTINEL), case.name
        assert torch.equal(out, plain) and not (spec2 == chk.SENTINEL).any()
        # fused FOA pass
        out, out_buf = _guarded((n, frames, 7, 64), torch.float32, gpu_device, chk.SENTINEL)
        with torch.cuda.device(index):
            seld_native.check(getattr(lib, f"seld_logmel_iv_{suffix}")(seld_native._p(pcm), n, length, seld_native._p(out), frames * 7 * 64,
                                                                      64, 1, 7 * 64, stream), "seld_logmel_iv")
        assert _guards_intact(out_buf, chk.SENTINEL) and not (out == chk.SENTINEL).any(), case.name
