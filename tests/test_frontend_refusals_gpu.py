"""GPU check of what the 16 front-end entry points refuse, with which code, which ``seld_last_error()`` text and in which
order: the 12 exports of csrc/logmel.hip, seld_foa_intensity, seld_gcc_phat, seld_gcc_phat_q15 and seld_nipd_q15.  The
codes and texts are those of the commit before the launchers and entry points took their checks from shared functions.
Every call in the table is refused before anything is launched, so its pointers are one 256-byte buffer; the cases named
"a + b" have two bad arguments and pin which check comes first.  After an entry point's refusals a good call of its family
still succeeds.  The refusal of a device seld_init was never called for needs a process of its own."""
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

INVALID, NOT_INITIALISED, UNSUPPORTED = -1, -3, -4
BUF = "buf"                                 # a pointer argument: the 256-byte device buffer (+ n: n bytes into it)
STRIDES = {"sN": 4096, "sC": 64, "sM": 1, "sT": 512}
DEFAULTS = dict(pcm=BUF, spec=BUF, words=BUF, table=BUF, out=BUF, N=1, C=2, L=481, F=4, layout=0, **STRIDES)
SIGNATURES = {
    "seld_logmel": ("pcm", "N", "C", "L", "out", "layout"),
    "seld_logmel_strided": ("pcm", "N", "C", "L", "out", "sN", "sC", "sM", "sT"),
    "seld_logmel_export": ("pcm", "N", "C", "L", "out", "sN", "sC", "sM", "sT", "spec"),
    "seld_logmel_iv": ("pcm", "N", "L", "out", "sN", "sC", "sM", "sT"),
    "seld_stft": ("pcm", "N", "C", "L", "out"),
    "seld_foa_intensity": ("spec", "N", "F", "out", "sN", "sC", "sM", "sT"),
    "seld_gcc_phat": ("spec", "N", "C", "F", "out", "sN", "sC", "sM", "sT"),
    "seld_gcc_phat_q15": ("words", "N", "C", "F", "out", "sN", "sC", "sM", "sT"),
    "seld_nipd_q15": ("words", "N", "C", "F", "table", "out", "sN", "sC", "sM", "sT"),
}
# entry point -> (signature, message prefix, family of the good call)
ENTRIES = {
    "seld_logmel_f32": ("seld_logmel", "seld_logmel", "logmel"),
    "seld_logmel_i16": ("seld_logmel", "seld_logmel", "logmel"),
    "seld_logmel_f32_strided": ("seld_logmel_strided", "seld_logmel", "logmel"),
    "seld_logmel_i16_strided": ("seld_logmel_strided", "seld_logmel", "logmel"),
    "seld_logmel_spectrum_f32": ("seld_logmel_export", "seld_logmel", "logmel"),
    "seld_logmel_spectrum_i16": ("seld_logmel_export", "seld_logmel", "logmel"),
    "seld_logmel_phasors_f32": ("seld_logmel_export", "seld_logmel", "logmel"),
    "seld_logmel_phasors_i16": ("seld_logmel_export", "seld_logmel", "logmel"),
    "seld_logmel_iv_f32": ("seld_logmel_iv", "seld_logmel_iv", "logmel_iv"),
    "seld_logmel_iv_i16": ("seld_logmel_iv", "seld_logmel_iv", "logmel_iv"),
    "seld_stft_f32": ("seld_stft", "seld_stft", "stft"),
    "seld_stft_i16": ("seld_stft", "seld_stft", "stft"),
    "seld_foa_intensity": ("seld_foa_intensity", "seld_foa_intensity", "logmel_iv"),
    "seld_gcc_phat": ("seld_gcc_phat", "seld_gcc_phat", "logmel_gcc"),
    "seld_gcc_phat_q15": ("seld_gcc_phat_q15", "seld_gcc_phat_q15", "logmel_gcc"),
    "seld_nipd_q15": ("seld_nipd_q15", "seld_nipd_q15", "logmel_nipd"),
}
NULL = (INVALID, "null pointer")
REFLECT = (INVALID, "reflect padding needs L > n_fft/2 = 480 samples")
TOO_LONG = (UNSUPPORTED, "at most 2^30 samples per channel")
N_AND_C = (INVALID, "N and C must be positive")
N_AND_F = (INVALID, "N and F must be positive")
CHANNELS = (UNSUPPORTED, "2..8 channels")
WORDS = (UNSUPPORTED, "a clip's phasors exceed 2^31 words")
FRAMES = (UNSUPPORTED, "more than 2^31 frames")
LAG_ROWS = (UNSUPPORTED, "needs unit lag stride and 16-byte aligned rows")
BAND_ROWS = (UNSUPPORTED, "needs unit band stride and 16-byte aligned rows")
# a clip of 8 channels past 2^31 spectrum values (481 per row) / phasor words (488 per row); N F + 4096 at 2^31
CLIP_SPECTRA, CLIP_WORDS = dict(C=8, F=2 ** 31 // (8 * 481) + 1), dict(C=8, F=2 ** 31 // (8 * 488) + 1)
MANY_FRAMES = dict(N=2 ** 21 - 4, F=1024)


def _logmel(pointers):
    rows = [({name: None}, NULL) for name in pointers]
    rows += [(dict(N=0), N_AND_C), (dict(C=0), N_AND_C), (dict(N=-1, C=-1), N_AND_C)]
    rows += [(dict(L=480), REFLECT), (dict(L=1), REFLECT), (dict(L=2 ** 30), TOO_LONG)]
    rows += [(dict(pcm=None, N=0), NULL), (dict(out=None, L=480), NULL), (dict(C=0, L=480), N_AND_C), (dict(N=0, L=2 ** 30), N_AND_C)]
    return rows


def _rows_refused(why):
    return [(dict(sM=2), why), (dict(out=(BUF, 4)), why), (dict(sN=4098), why), (dict(sC=66), why), (dict(sT=510), why)]


def _pairs(first, clip, clip_why):
    rows = [({first: None}, NULL), (dict(out=None), NULL), (dict(N=0), N_AND_F), (dict(F=0), N_AND_F), (dict(N=-3, F=-1), N_AND_F)]
    rows += [(dict(C=1), CHANNELS), (dict(C=9), CHANNELS), (dict(C=0), CHANNELS), (clip, clip_why)]
    rows += [({first: None, "C": 1}, NULL), (dict(N=0, C=9), N_AND_F), (dict(C=9, F=2 ** 40), CHANNELS)]
    return rows


TABLE = {
    "seld_logmel": _logmel(("pcm", "out")) + [
        (dict(layout=2), (INVALID, "layout must be 0 or 1")), (dict(layout=-1), (INVALID, "layout must be 0 or 1")),
        (dict(layout=2, L=2 ** 30), TOO_LONG), (dict(layout=2, N=0), N_AND_C)],
    "seld_logmel_strided": _logmel(("pcm", "out")),
    "seld_logmel_export": _logmel(("pcm", "out", "spec")) + [(dict(spec=None, C=0), NULL)],
    "seld_logmel_iv": [
        (dict(pcm=None), NULL), (dict(out=None), NULL), (dict(N=0), (INVALID, "N must be positive")),
        (dict(N=-2), (INVALID, "N must be positive")), (dict(L=480), REFLECT), (dict(L=2 ** 30), TOO_LONG),
        (dict(pcm=None, N=0), NULL), (dict(N=0, L=480), (INVALID, "N must be positive"))],
    "seld_stft": _logmel(("pcm", "out")),
    "seld_foa_intensity": [
        (dict(spec=None), NULL), (dict(out=None), NULL), (dict(N=0), N_AND_F), (dict(F=0), N_AND_F),
        (dict(spec=None, F=0), NULL)],
    "seld_gcc_phat": _pairs("spec", CLIP_SPECTRA, (UNSUPPORTED, "a clip's spectra exceed 2^31 complex values")),
    "seld_gcc_phat_q15": _pairs("words", CLIP_WORDS, WORDS) + [(MANY_FRAMES, FRAMES)] + _rows_refused(LAG_ROWS) + [
        (dict(CLIP_WORDS, N=2 ** 31), WORDS), (dict(MANY_FRAMES, sM=2), FRAMES), (dict(C=9, sM=2), CHANNELS)],
    "seld_nipd_q15": _pairs("words", CLIP_WORDS, WORDS) + [(dict(table=None), NULL), (MANY_FRAMES, FRAMES)]
    + _rows_refused(BAND_ROWS) + [
        (dict(words=(BUF, 4)), (UNSUPPORTED, "phasor rows must be 16-byte aligned, the table 4-byte aligned")),
        (dict(table=(BUF, 2)), (UNSUPPORTED, "phasor rows must be 16-byte aligned, the table 4-byte aligned")),
        (dict(CLIP_WORDS, N=2 ** 31), WORDS), (dict(MANY_FRAMES, sM=2), FRAMES), (dict(words=(BUF, 4), sM=2), BAND_ROWS)],
}


def _arguments(signature, changes, buffer):
    values = dict(DEFAULTS, **changes)
    args = []
    for name in SIGNATURES[signature]:
        v = values[name]
        if v == BUF:
            v = buffer.data_ptr()
        elif isinstance(v, tuple):
            v = buffer.data_ptr() + v[1]
        args.append(v)
    return args


def _good_call(nat, family, device, int16):
    g = torch.Generator().manual_seed(3)
    channels = {"logmel": 2, "stft": 2, "logmel_iv": 4, "logmel_gcc": 3, "logmel_nipd": 3}[family]
    pcm = torch.rand(1, channels, 481, generator=g) - 0.5
    pcm = (torch.round(pcm * 32767.0).to(torch.int16) if int16 else pcm).to(device)
    if family == "logmel":
        return nat.logmel(pcm)
    if family == "stft":
        return torch.view_as_real(nat.stft(pcm))
    return nat.spatial_features(pcm, family)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals_have_the_parent_codes_texts_and_order(gpu_device, entry):
    import seld_native as nat
    signature, prefix, family = ENTRIES[entry]
    nat.ensure_init(gpu_device)
    lib, stream = nat.load_library(), nat._stream_ptr(gpu_device)
    buffer = torch.zeros(64, device=gpu_device)
    assert any(len(changes) >= 2 for changes, _ in TABLE[signature])
    for changes, (code, why) in TABLE[signature]:
        rc = getattr(lib, entry)(*_arguments(signature, changes, buffer), stream)
        assert (rc, lib.seld_last_error().decode()) == (code, f"{prefix}: {why}"), (entry, changes)
    torch.cuda.synchronize(gpu_device)
    assert not buffer.any()                                          # nothing ran on the 256 bytes
    assert torch.isfinite(_good_call(nat, family, gpu_device, entry.endswith("i16"))).all()


_UNINITIALISED = """
import sys
sys.path[:0] = {path!r}
import test_frontend_refusals_gpu as t
import seld_native as nat
lib = nat.load_library()                    # (load_library does not call seld_init)

class Fake:
    def data_ptr(self):
        return 0x1000

for entry, (signature, prefix, family) in sorted(t.ENTRIES.items()):
    rc = getattr(lib, entry)(*t._arguments(signature, dict(), Fake()), None)
    text = lib.seld_last_error().decode()
    assert (rc, text) == (t.NOT_INITIALISED, "seld_init(device) has not been called for the current device"), (entry, rc, text)
print("refused", len(t.ENTRIES))
"""


def test_every_entry_point_refuses_a_device_without_seld_init(gpu_device):
    here = Path(__file__).resolve().parent
    path = [str(here), str(here.parent / "sound-event-localization-detection_amd")]
    done = subprocess.run([sys.executable, "-c", _UNINITIALISED.format(path=path)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip() == "refused 16", done.stdout + done.stderr
