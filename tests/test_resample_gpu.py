"""GPU checks of the sample-rate converter (csrc/resample.hip, seld_native.resample, dataset.py, infer.py) against the float64
restatement of DESIGN.md section 16.1 (tests/resample_ref.py).  Every test goes through seld_resample_f32 / _i16."""
import ctypes
import wave

import numpy as np
import pytest
import torch

import resample_ref as ref

pytestmark = pytest.mark.gpu

IMPULSE_RATES = (48000, 44100, 16000, 11025)
RANDOM_RATES = (48000, 44100, 32000, 16000, 11025, 96000)
# 1 and 100: shorter than the filter; 4801: a ragged end; 20011: several workgroups at every rate.  A workgroup takes a run of
# outputs that is a whole number of input samples: 2048 outputs = 4096 inputs at 48 kHz, 80 x 64 = 5120 outputs = 9408
# inputs at 44.1 kHz -- 4097 and 9409 put exactly one output into the next workgroup
LENGTHS = (1, 100, 4801, 20011, 4097, 9409)
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def native(gpu_device):
    import seld_native
    seld_native.ensure_init(gpu_device)
    return seld_native


_prototypes = {}


def _prototype(rate):
    if rate not in _prototypes:
        _prototypes[rate] = ref.prototype(rate)
    return _prototypes[rate]


def _expected_impulse(table, rate, length, k, amplitude):
    """The table entry the definition assigns to every output sample of an impulse at input sample k."""
    up, down, taps, half, _ = ref.plan(rate)
    m = np.arange(ref.output_length(length, rate), dtype=np.int64)
    p, q = (m * down) % up, (m * down) // up
    t = q - k + half                                            # x[q - (t - half)] is the impulse
    inside = (t >= 0) & (t < taps)
    return np.where(inside, table[p, np.clip(t, 0, taps - 1)], np.float32(0.0)) * np.float32(amplitude)


@pytest.mark.parametrize("dtype", ["fp32", "int16"])
@pytest.mark.parametrize("rate", IMPULSE_RATES)
def test_impulses_return_the_table_bit_for_bit(native, gpu_device, rate, dtype):
    length = 4801
    positions = (0, 1, length // 2, length - 1)
    table, _ = native.resample_table(rate)
    x = np.zeros((1, len(positions), length), dtype=np.float32 if dtype == "fp32" else np.int16)
    for c, k in enumerate(positions):
        x[0, c, k] = 1.0 if dtype == "fp32" else 16384
    got = native.resample(torch.from_numpy(x).to(gpu_device), rate).cpu().numpy()
    assert got.shape == (1, len(positions), ref.output_length(length, rate)) and got.dtype == np.float32
    for c, k in enumerate(positions):
        want = _expected_impulse(table, rate, length, k, 1.0 if dtype == "fp32" else 0.5)
        assert np.count_nonzero(want) > 10
        assert np.array_equal(got[0, c], want), (rate, dtype, k, int(np.flatnonzero(got[0, c] != want)[0]))
    # the same entries from the float64 restatement: |i| <= n, zero outside
    g, n = _prototype(rate)
    up, down, *_ = ref.plan(rate)
    k = positions[2]
    i = np.arange(got.shape[-1], dtype=np.int64) * down - k * up
    dense = np.where(np.abs(i) <= n, g[np.clip(i + n, 0, 2 * n)], 0.0) * (1.0 if dtype == "fp32" else 0.5)
    assert np.abs(got[0, 2] - dense).max() <= 2.0 ** -24 * up * 1.0001 and np.array_equal(got[0, 2] == 0, dense == 0)


@pytest.fixture(scope="module")
def random_pcm():
    """int16 [2, 3, 20011]; the fp32 signal is the same samples / 32768 (exact), so one float64 reference serves both."""
    rng = np.random.default_rng(20)
    return (rng.standard_normal((2, 3, max(LENGTHS))) * 6000).clip(-32768, 32767).astype(np.int16)


_references = {}


def _reference(random_pcm, rate, length):
    key = (rate, length)
    if key not in _references:
        out_len = ref.output_length(length, rate)
        _references[key] = ref.resample_at(random_pcm[..., :length], rate, np.arange(out_len), g_n=_prototype(rate),
                                           scale=1.0 / 32768.0)
    return _references[key]


@pytest.mark.parametrize("dtype", ["fp32", "int16"])
@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("rate", RANDOM_RATES)
def test_random_signals_against_float64(native, gpu_device, random_pcm, rate, length, dtype):
    taps = ref.plan(rate)[2]
    x16 = np.ascontiguousarray(random_pcm[..., :length])
    x = torch.from_numpy(x16) if dtype == "int16" else torch.from_numpy(x16.astype(np.float32) / np.float32(32768.0))
    got = native.resample(x.to(gpu_device), rate).cpu().numpy().astype(np.float64)
    want, b = _reference(random_pcm, rate, length)
    assert got.shape == want.shape == (2, 3, ref.output_length(length, rate))
    bound = (taps + 2) * EPS * b
    excess = np.abs(got - want) - bound
    used = (np.abs(got - want) / np.maximum(bound, 1e-300)).max()
    print(f"{rate} Hz, L = {length}, {dtype}: {used:.3f} of the bound")
    assert (excess <= 0).all(), (rate, length, dtype, float(used))
    assert np.abs(want).max() > 0.01


def test_indices_past_2_to_the_31(native, gpu_device):
    rate, length = 44100, 27_000_000
    up, down, taps, half, _ = ref.plan(rate)
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-20000, 20000, (1, 1, length), dtype=torch.int16, generator=g)
    got = native.resample(x.to(gpu_device), rate)
    out_len = ref.output_length(length, rate)
    assert got.shape == (1, 1, out_len)
    wrap = -(-2 ** 31 // down)                                  # the first m with m * down >= 2^31
    assert (out_len - 1) * down > 2 ** 31 + 2048 * down
    for name, first in (("head", 0), ("wrap", wrap - 2048), ("tail", out_len - 4096)):
        idx = np.arange(first, first + 4096)
        want, b = ref.resample_at(x.numpy()[0, 0], rate, idx, g_n=_prototype(rate), scale=1.0 / 32768.0)
        have = got[0, 0, first:first + 4096].cpu().numpy().astype(np.float64)
        used = (np.abs(have - want) / ((taps + 2) * EPS * b)).max()
        print(f"{name}: {used:.3f} of the bound")
        assert used <= 1.0, (name, float(used))
        assert np.abs(want).max() > 0.01


@pytest.mark.parametrize("rate", [48000, 44100])
def test_rows_are_independent(native, gpu_device, random_pcm, rate):
    x = torch.from_numpy(np.ascontiguousarray(random_pcm[..., :4801])).to(gpu_device)
    whole = native.resample(x, rate)
    for n in range(2):
        for c in range(3):
            alone = native.resample(x[n:n + 1, c:c + 1].contiguous(), rate)
            assert torch.equal(alone[0, 0], whole[n, c]), (n, c)
    two_d = native.resample(x[1].contiguous(), rate)            # [C, L] in, [C, L_out] out
    assert two_d.shape == whole.shape[1:] and torch.equal(two_d, whole[1])
    out = torch.full_like(whole, float("nan"))
    assert native.resample(x, rate, out=out) is out and torch.equal(out, whole)
    out2 = torch.full_like(whole[0], float("nan"))              # [C, L] in takes a [C, L_out] buffer
    native.resample(x[0].contiguous(), rate, out=out2)
    assert torch.equal(out2, whole[0])


def test_argument_checks(native, gpu_device):
    x = torch.zeros(1, 2, 1000, device=gpu_device)
    with pytest.raises(native.SeldNativeError):
        native.resample(torch.zeros(1, 2, 1000), 48000)                           # a host tensor
    with pytest.raises(ValueError):
        native.resample(torch.zeros(1, 1000, 2, device=gpu_device).transpose(1, 2), 48000)      # not contiguous
    with pytest.raises(TypeError):
        native.resample(x.to(torch.float64), 48000)
    with pytest.raises(native.SeldNativeError, match="44056"):
        native.resample(x, 44056)                                                 # not a supported rate
    with pytest.raises(ValueError):
        native.resample(x, 48000, out=torch.zeros(1, 2, 501, device=gpu_device))
    with pytest.raises(ValueError):
        native.resample(torch.zeros(1000, device=gpu_device), 48000)
    # the C entry point itself: a wrong output length, taps != 2 half + 1 and a null table launch nothing
    lib = native.load_library()
    (up, down, taps, half), table = native._resample_table_device(48000, 24000, gpu_device, gpu_device.index or 0)
    out = torch.full((1, 2, 500), 7.0, device=gpu_device)
    stream = native._stream_ptr(gpu_device)

    def call(table_ptr, taps_, out_len):
        return lib.seld_resample_f32(ctypes.c_void_p(x.data_ptr()), 1, 2, 1000, table_ptr, up, down, taps_, half,
                                     ctypes.c_void_p(out.data_ptr()), out_len, stream)
    good = ctypes.c_void_p(table.data_ptr())
    assert call(good, taps, 499) == -1 and b"500" in lib.seld_last_error()
    assert call(good, taps - 1, 500) == -1
    assert call(None, taps, 500) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call(good, taps, 500) == 0
    torch.cuda.synchronize()
    assert (out == 0.0).all()


@pytest.fixture
def resample_switch():
    """Config.RESAMPLE_INPUT as the dataset path reads it; whatever a test sets is removed afterwards."""
    import dataset
    had = "RESAMPLE_INPUT" in vars(dataset.config)
    saved = vars(dataset.config).get("RESAMPLE_INPUT")

    def set_to(value):
        dataset.config.RESAMPLE_INPUT = value
    yield set_to
    if had:
        dataset.config.RESAMPLE_INPUT = saved
    elif "RESAMPLE_INPUT" in vars(dataset.config):
        del dataset.config.RESAMPLE_INPUT


def test_dataset_converts_when_the_switch_is_on(native, gpu_device, resample_switch):
    import dataset
    from oracle import labels as olab
    rng = np.random.default_rng(3)
    length = 100799                                             # 104 label frames; its 24 kHz conversion alone would have 105
    pcm48 = torch.from_numpy((rng.standard_normal((4, length)) * 3000).clip(-32768, 32767).astype(np.int16))
    rows = olab.synth_metadata(0, meta_frames=25)
    resample_switch(False)
    with pytest.raises(NotImplementedError, match="48000"):
        dataset.SELDDataset.from_pcm([pcm48], [rows], sample_rate=48000, device=gpu_device)
    resample_switch(True)
    ds48 = dataset.SELDDataset.from_pcm([pcm48], [rows], sample_rate=48000, device=gpu_device)
    pcm24 = native.resample(pcm48.to(gpu_device), 48000)
    assert pcm24.shape == (4, 50400) and pcm24.dtype == torch.float32
    ds24 = dataset.SELDDataset.from_pcm([pcm24], [rows], sample_rate=24000, device=gpu_device)
    frames = dataset.label_frame_count(length / 48000)
    assert frames == 104 and ds48.total_frames == frames        # the labels keep the file's duration
    assert ds24.total_frames == 105
    assert torch.equal(ds48.spec_tm, ds24.spec_tm[:frames])
    assert torch.equal(ds48.mask_tm, ds24.mask_tm[:frames])
    assert int((ds48.mask_tm != 0).sum()) > 0
    # audio_to_mel_spectrogram: the same conversion in front of the log-mel kernel; other FFT sizes still raise
    x = pcm48.to(gpu_device)
    assert torch.equal(dataset.audio_to_mel_spectrogram(x, 48000), native.logmel(pcm24, layout="cft"))
    with pytest.raises(NotImplementedError):
        dataset.audio_to_mel_spectrogram(x, 48000, n_fft=1024)
    resample_switch(False)
    with pytest.raises(NotImplementedError):
        dataset.audio_to_mel_spectrogram(x, 48000)


@pytest.fixture(scope="module")
def crnn_checkpoint(gpu_device, tmp_path_factory):
    """A seeded, untrained CRNN written in the trainer's checkpoint format."""
    import trainer
    old = trainer.config.MODEL_TYPE
    trainer.config.MODEL_TYPE = "crnn"
    torch.manual_seed(0)
    model = trainer.prepare_model_for_device(trainer.build_model((18, 36), True, n_channels=4), gpu_device)
    path = tmp_path_factory.mktemp("seld_resample") / "crnn.pth"
    torch.save({"epoch": 0, "model_state_dict": trainer.model_state_dict(model), "train_loss": 0.0, "test_loss": 0.0},
               path)
    yield path
    trainer.config.MODEL_TYPE = old


@pytest.fixture
def deterministic_convolutions():
    """MIOpen's default convolution solutions are not bitwise repeatable from call to call; its deterministic mode is."""
    saved = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved


def test_infer_cli_on_a_48_khz_recording(native, gpu_device, crnn_checkpoint, tmp_path, deterministic_convolutions,
                                         resample_switch):
    import dataset
    import infer
    import seld_eval
    import trainer
    from utils import safe_torch_load
    rng = np.random.default_rng(4)
    pcm = (rng.standard_normal((48000 * 6, 4)) * 3000).clip(-32768, 32767).astype("<i2")
    wav = tmp_path / "take_48k.wav"
    with wave.open(str(wav), "wb") as wf:
        wf.setnchannels(4)
        wf.setsampwidth(2)
        wf.setframerate(48000)
        wf.writeframes(pcm.tobytes())
    threshold, max_peaks = 1.0 / 14.0 + 1e-4, 8
    common = ["--checkpoint", str(crnn_checkpoint), "--model-type", "crnn", "--threshold", str(threshold),
              "--max-peaks", str(max_peaks), "--device", str(gpu_device)]
    assert infer.parse_args(common + ["--out-dir", "x", str(wav)]).resample is False
    assert infer.parse_args(common + ["--out-dir", "x", "--resample", str(wav)]).resample is True
    with pytest.raises(NotImplementedError, match="48000"):
        infer.main(common + ["--out-dir", str(tmp_path / "off"), str(wav)])
    written = infer.main(common + ["--out-dir", str(tmp_path / "on"), "--resample", str(wav)])
    assert "RESAMPLE_INPUT" not in vars(dataset.config) or dataset.config.RESAMPLE_INPUT is False     # set for the run only
    got = dataset._read_metadata_rows(written[0])

    # the same events from the 24 kHz dataset built from seld_native.resample of the same PCM
    pcm24 = native.resample(torch.from_numpy(np.ascontiguousarray(pcm.T)).to(gpu_device), 48000)
    ds = dataset.SELDDataset.from_pcm([pcm24], [np.zeros((0, 5), dtype=np.int64)], sample_rate=24000, device=gpu_device,
                                      use_gaussian_augmentation=False)
    assert ds.total_frames == 300
    checkpoint = safe_torch_load(str(crnn_checkpoint), map_location=gpu_device)
    old = trainer.config.MODEL_TYPE
    trainer.config.MODEL_TYPE = "crnn"
    try:
        model = trainer.prepare_model_for_device(trainer.build_model((ds.I, ds.J), True, n_channels=ds.n_channels),
                                                 gpu_device)
    finally:
        trainer.config.MODEL_TYPE = old
    model.load_state_dict(trainer.select_state_dict(checkpoint, None))
    model.eval()
    result = seld_eval.evaluate_logits(trainer.timeline_logits(model, ds, trainer.config.BATCH_SIZE, gpu_device), ds,
                                       threshold=threshold, max_peaks=max_peaks, events_dir=tmp_path / "ref",
                                       names=["take_48k"], patterns=(), track=False, refine=False)
    want = dataset._read_metadata_rows(result["event_files"][0])
    assert want.shape[0] > 0 and want.shape[1] == 5
    assert np.array_equal(got, want)
    assert got[:, 0].min() >= 0 and got[:, 0].max() < 60        # 6 s = 60 meta-frames
