"""CPU tests of the front-end input families (tests/frontend_cases.py) and of the all-zero-frame rule of
csrc/logmel_core.h, the latter on the lane emulator (tests/emu/logmel_emu.cpp, a TEST tool).

Premises, in float64 against oracle/features.py: a family that stops exercising its case fails here, not silently.
Emulator: with the rule, every all-zero frame exports exact zeros in every slot of the packing and on both load paths,
and every other frame's words, spectra and dB values are bit for bit what the core without the rule produces; the
emulator's outputs then go through the same checks as the GPU's (tests/frontend_checks.py)."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import frontend_cases as fc
import frontend_checks as chk
import nipd_ref
from oracle import features as ofeat

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "sound-event-localization-detection_amd"
EMU_SRC = ROOT / "tests" / "emu" / "logmel_emu.cpp"
EMU_LIB = ROOT / "tests" / "emu" / "libseld_emu.so"
CORE = PKG / "csrc" / "logmel_core.h"

SILENCE = ofeat.GCC_SILENCE_POWER
FAR_ABOVE = 100.0 * SILENCE                      # a sounding frame's weakest bin
LOUD_BIN = 1e3                                   # the partner of an all-zero frame has a bin at least this strong
ALL_FAMILIES = ((fc.loud_gap, 8), (fc.loud_gap, 2), (fc.loud_gap_one_channel, 6), (fc.loud_gap_one_channel, 7),
                (fc.full_scale_i16, 8), (fc.scaled, 8), (fc.scaled, 4))


def _all_cases():
    return [(family, case) for family, channels in ALL_FAMILIES for case in family(channels)]


def _power(case):
    spec = ofeat.stft_f64(fc.as_float(case).astype(np.float64))                   # [C, 481, F]
    return (spec.real ** 2 + spec.imag ** 2).transpose(0, 2, 1)                    # [C, F, 481]


def _interior(case, t):
    """Frame t lies in an iteration that takes the interior load path (csrc/logmel.hip launch_logmel)."""
    itr = t // 4
    return itr >= 1 and 480 * (4 * itr + 4) <= case.pcm.shape[1]


# ---------------------------------------------------------------------------------------------------- premises

def test_frame_counts_and_remainders():
    for family in (fc.loud_gap, fc.loud_gap_one_channel):
        cases = family(4)
        frames = {c.frames for c in cases}
        assert set(range(2, 10)) <= frames and frames & {17, 18, 19, 20}
        assert {c.pcm.shape[1] % 480 for c in cases} == {0, 1, 479}
        assert {c.frames % 4 for c in cases} == {0, 1, 2, 3}
        assert {c.carrier for c in cases} == set(fc.CARRIERS)
    assert [c.name for c in fc.loud_gap(4)] == [c.name for c in fc.loud_gap(4)]
    again = fc.carrier("tone_between", 500, 9001)
    assert np.array_equal(again, fc.carrier("tone_between", 500, 9001))           # deterministic from the seed


def test_every_frame_is_all_zero_or_far_above_the_silence_threshold():
    for _, case in _all_cases():
        power = _power(case)
        dead = fc.dead_frames(case.pcm)
        assert not power[dead].any(), case.name                                    # float64 agrees: spectrum exactly 0
        assert power[~dead].min() >= FAR_ABOVE, (case.name, power[~dead].min())


def test_no_sounding_frame_is_far_below_its_packing_partner():
    """fp32 cannot resolve a frame 140 dB under its packing partner: level steps are excluded, every
    sounding frame is within 40 dB of the frame it is packed with."""
    for _, case in _all_cases():
        energy = _power(case).sum(axis=2)                                          # [C, F]
        dead = fc.dead_frames(case.pcm)
        for t in range(case.frames):
            q = t ^ 1
            if q < case.frames:
                both = ~dead[:, t] & ~dead[:, q]
                assert (energy[both, t] >= 1e-4 * energy[both, q]).all(), (case.name, t)


@pytest.mark.parametrize("family,channels", [(fc.loud_gap, 4), (fc.loud_gap_one_channel, 7), (fc.full_scale_i16, 4)])
def test_all_zero_frames_sit_next_to_loud_partners_in_every_slot(family, channels):
    slots, first, last, interior, boundary = set(), False, False, set(), set()
    for case in family(channels):
        peak = _power(case).max(axis=2)                                            # [C, F]
        dead = fc.dead_frames(case.pcm)
        for c, t in zip(*np.nonzero(dead)):
            q = t ^ 1
            if q < case.frames and not dead[c, q] and peak[c, q] >= LOUD_BIN:
                slots.add(t % 4)
                first |= t < 4
                last |= t // 4 == (case.frames - 1) // 4
                if _interior(case, t):
                    interior.add(t % 4)
                if t >= 4:
                    boundary.add(t % 4)
    assert slots == {0, 1, 2, 3} and first and last
    assert interior == {0, 1, 2, 3}                                                # both load paths, both pairs, both slots
    assert {0, 3} <= boundary                                                      # either side of an iteration boundary


def test_first_iteration_starts_with_zeros_and_the_clip_end_is_zero_padded():
    cases = fc.loud_gap(2)
    assert any(not c.pcm[:, :481].any() and fc.dead_frames(c.pcm)[:, 0].all() for c in cases)
    ends = [c for c in cases if fc.dead_frames(c.pcm)[:, -1].all()]
    assert {c.frames % 4 for c in ends} >= {1, 2, 3}                               # partial last iterations of 1, 2, 3 frames
    assert any(c.frames % 4 == 0 for c in ends)


@pytest.mark.parametrize("channels", [6, 7])
def test_one_channel_family_mixes_silent_and_sounding_channels(channels):
    """15 and 21 pairs: either side of the GCC kernels' 16-pair tile."""
    for case in fc.loud_gap_one_channel(channels):
        dead = fc.dead_frames(case.pcm)
        mixed = dead.any(axis=0) & ~dead.all(axis=0)
        assert mixed.any() and not dead.all(axis=0).any(), case.name
        assert dead[[1, 4]].any(axis=1).all() and not dead[[0, 2, 3, 5]].any()


def test_full_scale_i16_reaches_both_ends_of_the_range():
    for case in fc.full_scale_i16(4):
        assert case.pcm.dtype == np.int16 and case.pcm.min() == -32768 and case.pcm.max() == 32767
        assert fc.dead_frames(case.pcm).all(axis=0).any()
        assert fc.as_float(case).min() == -1.0


def test_scaled_family_is_exact_power_of_two_copies():
    cases = fc.scaled(4)
    assert sorted({c.scale_log2 for c in cases}) == [0, 4, 10]
    for base in (c for c in cases if c.scale_log2 == 0):
        assert np.abs(base.pcm).max() > 0.9
        for c in cases:
            if c.pcm.shape == base.pcm.shape and c.scale_log2:
                assert np.array_equal(c.pcm.astype(np.float64) * 2.0 ** c.scale_log2, base.pcm.astype(np.float64))


@pytest.mark.parametrize("family,channels", [(fc.loud_gap, 8), (fc.full_scale_i16, 4)])
def test_planted_delay_is_the_float64_peak(family, channels):
    hits = 0
    for case in family(channels):
        r = chk.ref_of(case, family)
        gcc, _ = r.gcc()
        sounding = ~r.dead.any(axis=0)
        for t in range(1, r.frames - 1):
            if sounding[t - 1:t + 2].all():
                for p, (m, n) in enumerate(chk.pairs(channels)):
                    assert gcc[p, :, t].argmax() == 32 + case.delays[n] - case.delays[m], (case.name, t, m, n)
                    hits += 1
    assert hits >= 30


# ---------------------------------------------------------------------------------------------------- the emulator

@pytest.fixture(scope="module")
def emu():
    newest = max(EMU_SRC.stat().st_mtime, CORE.stat().st_mtime)
    if not EMU_LIB.exists() or EMU_LIB.stat().st_mtime < newest:
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I", str(PKG / "csrc"),
                        str(EMU_SRC), "-o", str(EMU_LIB)], check=True)
    lib = ctypes.CDLL(str(EMU_LIB))
    lib.emu_phasor_pitch.restype = ctypes.c_int64
    return lib


_FB = np.ascontiguousarray(ofeat.mel_filterbank_htk().numpy())


def _export(emu, pcm, kind, rule):
    """The emulator's phasor ('phasors') or spectrum ('spectrum') pass on pcm [C, L] with the C ABI's arguments:
    (log-mel [C, 64, F], words int32 [C, F, pitch] or spectrum complex64 [C, F, 481]); buffers pre-filled with sentinels."""
    c, length = pcm.shape
    frames = 1 + length // 480
    x = np.ascontiguousarray(pcm)
    suffix = "f32" if x.dtype == np.float32 else "i16"
    out = np.full((frames, c, 64), chk.SENTINEL, np.float32)
    if kind == "phasors":
        side = np.full((c, frames, int(emu.emu_phasor_pitch())), -1, np.int32)
    else:
        side = np.full((c, frames, 481, 2), chk.SENTINEL, np.float32)
    fn = getattr(emu, f"emu_logmel_{kind}_{suffix}")
    i64 = ctypes.c_int64
    rc = fn(ctypes.c_void_p(x.ctypes.data), i64(1), i64(c), i64(length), ctypes.c_void_p(out.ctypes.data), i64(frames * c * 64),
            i64(64), i64(1), i64(c * 64), ctypes.c_void_p(side.ctypes.data), ctypes.c_void_p(_FB.ctypes.data), ctypes.c_int(rule))
    assert rc == 0                                                                 # (-9: an LDS index left the tile)
    assert not (out == chk.SENTINEL).any()
    if kind == "spectrum":
        assert not (side == chk.SENTINEL).any()
        side = side.view(np.complex64)[..., 0]
    return out.transpose(1, 2, 0), side


def _iv(emu, pcm, rule):
    frames = 1 + pcm.shape[1] // 480
    x = np.ascontiguousarray(pcm[None].astype(np.float32))
    out = np.full((1, frames, 7, 64), chk.SENTINEL, np.float32)
    rc = emu.emu_logmel_iv_rule_f32(ctypes.c_void_p(x.ctypes.data), ctypes.c_int64(1), ctypes.c_int64(pcm.shape[1]),
                                    ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(_FB.ctypes.data), ctypes.c_int(rule))
    assert rc == 0 and not (out == chk.SENTINEL).any()
    return out[0].transpose(1, 2, 0)                                               # [7, 64, F]


def test_emulator_exports_agree_with_the_plain_pass_and_the_oracle(emu):
    """The new entry points on plain noise: the log-mel channels are those of emu_logmel_*, the spectrum is float64's to
    the STFT bar, and the words of the strong bins are the spectrum's phasors to one Q15 step."""
    pcm = ofeat.synth_pcm(3, 3, 4800 + 7, "noise").numpy()
    db_w, words = _export(emu, pcm, "phasors", 1)
    db_s, spec = _export(emu, pcm, "spectrum", 1)
    assert np.array_equal(db_w, db_s)
    plain = np.full((3, 64, 11), np.nan, np.float32)
    assert emu.emu_logmel_f32(ctypes.c_void_p(np.ascontiguousarray(pcm).ctypes.data), ctypes.c_int64(1), ctypes.c_int64(3),
                              ctypes.c_int64(pcm.shape[1]), ctypes.c_void_p(plain.ctypes.data), ctypes.c_int(0),
                              ctypes.c_void_p(_FB.ctypes.data)) == 0
    assert np.array_equal(plain, db_w)
    ref = np.swapaxes(ofeat.stft_f64(pcm.astype(np.float64)), -1, -2)
    assert np.abs(spec - ref).max() <= chk.STFT_REL * np.abs(ref).max()
    re, im = nipd_ref.words_to_int(words[..., :481])
    unit = ref / np.abs(ref)
    strong = np.abs(ref) >= 0.05 * np.abs(ref).max()          # (a weak bin's phase carries the transform's fp32 error)
    assert strong.mean() > 0.5
    assert np.abs(re - 32767.0 * unit.real)[strong].max() <= 1.0 and np.abs(im - 32767.0 * unit.imag)[strong].max() <= 1.0
    assert (words[..., 481:] == -1).all()


@pytest.mark.parametrize("family,channels", [(fc.loud_gap, 2), (fc.loud_gap_one_channel, 2), (fc.full_scale_i16, 2)])
def test_all_zero_frames_export_exact_zeros_and_nothing_else_changes(emu, family, channels):
    leaked = 0
    for case in family(channels):
        dead = fc.dead_frames(case.pcm)
        db1, words1 = _export(emu, case.pcm, "phasors", 1)
        db0, words0 = _export(emu, case.pcm, "phasors", 0)
        _, spec1 = _export(emu, case.pcm, "spectrum", 1)
        _, spec0 = _export(emu, case.pcm, "spectrum", 0)
        # with the rule: exact zeros in every all-zero frame, whichever slot and load path it is in
        assert not words1[dead][:, :481].any(), case.name
        assert not spec1[dead].view(np.float32).any(), case.name
        assert (db1.transpose(0, 2, 1)[dead] == -100.0).all(), case.name
        # every other frame: bit for bit the core without the rule
        live = ~dead
        assert np.array_equal(words1[live], words0[live]), case.name
        assert np.array_equal(spec1[live].view(np.uint32), spec0[live].view(np.uint32)), case.name
        assert np.array_equal(db1.transpose(0, 2, 1)[live].view(np.uint32), db0.transpose(0, 2, 1)[live].view(np.uint32))
        assert (words1[..., 481:] == -1).all()                                     # the row's padding words are never written
        leaked += int(words0[dead][:, :481].any(axis=1).sum())
        chk.check_words_dead(chk.ref_of(case, family), words1)
    assert leaked > 0          # the comparison is not vacuous: without the rule these inputs do put words into silent frames


def test_fused_foa_pass_all_zero_frames(emu):
    for case in fc.loud_gap(4) + fc.loud_gap_one_channel(4):
        dead = fc.dead_frames(case.pcm)
        got1, got0 = _iv(emu, case.pcm, 1), _iv(emu, case.pcm, 0)
        assert (got1[:4].transpose(0, 2, 1)[dead] == -100.0).all(), case.name
        assert not got1[4:][:, :, dead.all(axis=0)].any(), case.name
        live = ~dead.any(axis=0)
        assert np.array_equal(got1[:, :, live].view(np.uint32), got0[:, :, live].view(np.uint32)), case.name


# The emulator's outputs through the checks the GPU's outputs go through (tests/test_frontend_edges_gpu.py): the host
# build's arithmetic is the device's up to fma contraction, so a family whose tolerance cannot hold shows here first.

@pytest.mark.parametrize("family,channels", [(fc.loud_gap, 4), (fc.loud_gap_one_channel, 7), (fc.full_scale_i16, 4),
                                             (fc.scaled, 4)])
def test_emulator_outputs_pass_the_front_end_checks(emu, family, channels):
    weights = chk.nipd_weights()
    for case in family(channels):
        r = chk.ref_of(case, family)
        db, words = _export(emu, case.pcm, "phasors", 1)
        _, spec = _export(emu, case.pcm, "spectrum", 1)
        figures = {}
        figures.update(chk.check_stft(r, spec))
        figures.update(chk.check_logmel(r, db))
        chk.check_words_dead(r, words)
        g = chk.check_gcc(r, chk.gcc_from_spec(chk.words_to_spec(words)), q15=True)
        figures.update({f"gcc_q15_{k}": v for k, v in g.items()})
        g = chk.check_gcc(r, chk.gcc_from_spec(np.swapaxes(spec, -1, -2)), q15=False)
        figures.update({f"gcc_spec_{k}": v for k, v in g.items()})
        n = chk.check_nipd(r, nipd_ref.nipd_from_words(words, weights))
        figures.update({f"nipd_{k}": v for k, v in n.items()})
        if channels == 4 and case.pcm.dtype == np.float32:
            i = chk.check_iv(r, _iv(emu, case.pcm, 1)[4:])
            figures.update({f"iv_{k}": v for k, v in i.items()})
        print(case.name, " ".join(f"{k}={v:.2e}" for k, v in figures.items()))
