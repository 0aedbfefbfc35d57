"""CPU tests of the native library boundary: it loads, exports every symbol the header declares,
its host-side tables match the oracle, and the kernel's lane-level algorithm (run by the CPU lane
emulator, a TEST tool) matches the oracle.  No GPU compute calls here."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import features as ofeat
from logmel_checks import assert_logmel_close

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "sound-event-localization-detection_amd"
HEADER = ROOT / "include" / "seld_hip.h"
EMU_SRC = ROOT / "tests" / "emu" / "logmel_emu.cpp"
EMU_LIB = ROOT / "tests" / "emu" / "libseld_emu.so"


@pytest.fixture(scope="module")
def native_lib():
    lib_path = PKG / "libseld_hip.so"
    if not lib_path.exists():
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(str(lib_path))


@pytest.fixture(scope="module")
def emu_lib():
    if not EMU_LIB.exists() or EMU_LIB.stat().st_mtime < EMU_SRC.stat().st_mtime:
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I", str(PKG / "csrc"),
                        str(EMU_SRC), "-o", str(EMU_LIB)], check=True)
    return ctypes.CDLL(str(EMU_LIB))


def declared_symbols():
    text = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(seld_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported(native_lib):
    names = declared_symbols()
    assert len(names) >= 12
    for name in names:
        assert hasattr(native_lib, name), f"{name} declared in include/seld_hip.h but not exported"


def test_python_binding_declares_the_same_entry_points(native_lib):
    import seld_native
    lib = seld_native.load_library()
    for name in declared_symbols():
        assert getattr(lib, name).argtypes is not None, f"seld_native._declare sets no argtypes for {name}"


def test_product_path_has_no_cpu_fallback():
    import seld_native
    with pytest.raises(seld_native.SeldNativeError):
        seld_native.logmel(torch.zeros(4, 4800))
    src = "".join(p.read_text() for p in PKG.glob("*.py"))
    assert "import oracle" not in src and "from oracle" not in src


def test_default_tables_match_oracle(native_lib):
    win = np.zeros(960, np.float32)
    fb = np.zeros((481, 64), np.float32)
    b0 = np.zeros(64, np.int32)
    wd = np.zeros((24, 64), np.float32)
    wu = np.zeros((24, 64), np.float32)
    native_lib.seld_default_tables.argtypes = [ctypes.c_void_p] * 5
    rc = native_lib.seld_default_tables(win.ctypes.data, fb.ctypes.data, b0.ctypes.data, wd.ctypes.data, wu.ctypes.data)
    assert rc == 0
    # torch builds its window in fp32 (the host uploads that one via seld_set_window); the C++ default is
    # the double-precision value rounded once
    assert np.abs(win - torch.hann_window(960, periodic=True).numpy()).max() <= 2.5e-7
    ref_fb = ofeat.mel_filterbank_htk().numpy()
    assert np.abs(fb - ref_fb).max() <= 1e-5
    assert np.array_equal(fb > 0, ref_fb > 0)
    # the sparse per-lane decomposition reproduces fb exactly: bin b0[j]+i feeds filter j with wd and j+1 with wu
    rebuilt = np.zeros_like(fb)
    for j in range(64):
        for i in range(24):
            k = b0[j] + i
            if wd[i, j] != 0:
                rebuilt[k, j] = wd[i, j]
            if wu[i, j] != 0:
                rebuilt[k, j + 1] = wu[i, j]
    assert np.array_equal(rebuilt, fb)


def test_host_mel_table_equals_oracle_table():
    import seld_native
    assert torch.equal(seld_native.mel_filterbank(), ofeat.mel_filterbank_htk())


def _emu(emu_lib, pcm, layout=0):
    c, length = pcm.shape
    frames = 1 + length // 480
    x = np.ascontiguousarray(pcm.numpy())
    out = np.full((c, 64, frames) if layout == 0 else (frames, c, 64), np.nan, np.float32)
    fb = np.ascontiguousarray(ofeat.mel_filterbank_htk().numpy())
    fn = emu_lib.emu_logmel_f32 if x.dtype == np.float32 else emu_lib.emu_logmel_i16
    rc = fn(ctypes.c_void_p(x.ctypes.data), ctypes.c_int64(1), ctypes.c_int64(c), ctypes.c_int64(length),
            ctypes.c_void_p(out.ctypes.data), ctypes.c_int(layout), ctypes.c_void_p(fb.ctypes.data))
    assert rc == 0
    return out


@pytest.mark.parametrize("num_samples,seed", [(481, 2), (959, 2), (960, 2), (7680, 2), (7681, 2), (24123, 2),
                                              (96480, 2), (24000, 4)])
def test_lane_emulator_matches_oracle(emu_lib, num_samples, seed):
    # (24000, seed 4) contains a band 60 dB below its frame's peak: the fp32 noise-floor case of logmel_checks
    pcm = ofeat.synth_pcm(seed, 4 if seed == 4 else 2, num_samples, "noise")
    got = _emu(emu_lib, pcm)
    ref = ofeat.logmel_torch(pcm).numpy()
    assert_logmel_close(got, ref)


def test_lane_emulator_layouts_int16_and_floor(emu_lib):
    pcm = ofeat.synth_pcm(4, 3, 20000, "noise")
    a = _emu(emu_lib, pcm, 0)
    b = _emu(emu_lib, pcm, 1)
    assert np.array_equal(a.transpose(2, 0, 1), b)
    xi = ofeat.pcm_to_int16(pcm)
    assert_logmel_close(_emu(emu_lib, xi), ofeat.logmel_torch(ofeat.int16_to_pcm(xi)).numpy())
    assert (_emu(emu_lib, torch.zeros(1, 5000)) == -100.0).all()


@pytest.mark.parametrize("num_samples,seed", [(481, 5), (960, 5), (7681, 5), (24123, 6)])
def test_lane_emulator_fused_foa_pass_matches_oracle(emu_lib, num_samples, seed):
    """The fused FOA kernel's per-lane functions (csrc/logmel_core.h: phase_c_unpack, iv_publish, iv_compute, iv_store_rows)
    stepped on the CPU as four lock-step wavefronts with the kernel's LDS layout (four contiguous tiles + W's spectrum
    buffer, guard cells around them): log-mel channels as the plain emulation, intensity vectors against the float64 oracle
    to the 1e-4 of the GPU test -- edge iterations (reflection, frames past the end) included."""
    pcm = ofeat.synth_pcm(seed, 4, num_samples, "noise")
    pcm[1] = 0.7 * pcm[0] + 0.3 * pcm[1]
    pcm[:, num_samples // 2: num_samples // 2 + 100] = 0.0                 # a stretch of digital silence: eps carries it
    frames = 1 + num_samples // 480
    batch = torch.stack([pcm, ofeat.synth_pcm(seed + 10, 4, num_samples, "noise")])
    x = np.ascontiguousarray(batch.numpy())
    out = np.full((2, frames, 7, 64), np.nan, np.float32)
    fb = np.ascontiguousarray(ofeat.mel_filterbank_htk().numpy())
    rc = emu_lib.emu_logmel_iv_f32(ctypes.c_void_p(x.ctypes.data), ctypes.c_int64(2), ctypes.c_int64(num_samples),
                                   ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(fb.ctypes.data))
    assert rc == 0                                                         # (-9: an LDS index left the block)
    assert np.isfinite(out).all()
    for i in range(2):
        assert np.array_equal(out[i, :, :4].transpose(1, 2, 0), _emu(emu_lib, batch[i]))
        ref = ofeat.foa_intensity_f64(batch[i].numpy())                    # [3, 64, F]
        assert np.abs(out[i, :, 4:].transpose(1, 2, 0) - ref).max() <= 1e-4
    assert np.abs(ofeat.foa_intensity_f64(pcm.numpy())[0]).max() > 0.1
    if num_samples == 7681:                                                # the int16 instantiation's sample conversion
        xi = ofeat.pcm_to_int16(pcm)
        x16 = np.ascontiguousarray(xi.numpy()[None])
        out16 = np.full((1, frames, 7, 64), np.nan, np.float32)
        rc = emu_lib.emu_logmel_iv_i16(ctypes.c_void_p(x16.ctypes.data), ctypes.c_int64(1), ctypes.c_int64(num_samples),
                                       ctypes.c_void_p(out16.ctypes.data), ctypes.c_void_p(fb.ctypes.data))
        assert rc == 0
        ref16 = ofeat.foa_intensity_f64(ofeat.int16_to_pcm(xi).numpy())
        assert np.abs(out16[0, :, 4:].transpose(1, 2, 0) - ref16).max() <= 1e-4


def test_device_code_has_no_vcc_scc_select_miscompile(tmp_path):
    """hipcc (ROCm 7.2, gfx950) lowered a uniform 64-bit ``min(n - cell0, 256)`` in two instantiations of the loss
    kernel to ``v_cmp_lt_i64 vcc`` + ``s_cselect_b32`` WITHOUT copying VCC to SCC: the select then read the stale
    carry of the preceding subtraction and the ragged last tile was processed as a full one.  The source now uses
    32-bit extents there; this scans the ISA of every kernel file for the pattern so a re-appearance is caught on
    the CPU."""
    import re
    import subprocess
    from pathlib import Path
    csrc = Path(__file__).resolve().parent.parent / "sound-event-localization-detection_amd" / "csrc"
    scc_writer = re.compile(r"^\s*(s_cmp|s_and_|s_or_|s_xor_|s_andn2|s_orn2|s_bitcmp|s_add|s_sub|s_addc|s_subb|s_lshl|s_lshr|"
                            r"s_ashr|s_min|s_max|s_abs|s_not|s_bcnt|s_absdiff|s_nand|s_nor|s_xnor|s_bfe)")
    for src in sorted(csrc.glob("*.hip")):
        out = tmp_path / (src.stem + ".s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{csrc.parent.parent / 'include'}",
                        "-S", "--cuda-device-only", str(src), "-o", str(out)], check=True, capture_output=True)
        lines = out.read_text().splitlines()
        for i, line in enumerate(lines):
            if "s_cselect" not in line and "s_cbranch_scc" not in line:
                continue
            j = i - 1
            while j >= 0 and not scc_writer.match(lines[j]) and "s_cselect" not in lines[j] \
                    and not lines[j].strip().endswith(":"):
                j -= 1
            writer = lines[j].strip() if j >= 0 else ""
            wide_cmp = [x for x in lines[j + 1:i] if "v_cmp" in x and "64" in x]
            assert not (wide_cmp and writer.startswith(("s_sub", "s_add", "s_lsh"))), \
                f"{src.name}: '{line.strip()}' selects on the SCC of '{writer}' after '{wide_cmp[0].strip()}'"


def test_hot_kernels_do_not_spill():
    """Register claims of DESIGN.md checked on the CPU: the compiler's own resource report (-Rpass-analysis=kernel-resource-usage)
    of the feature and recurrence kernels must show NO scratch -- the round-2 review found 56 B per lane in
    ``logmel_main_kernel<float, 1>`` by recompiling; a spill in one of these is a silent 10 - 30 % on a tuned kernel."""
    import re
    import subprocess
    from concurrent.futures import ThreadPoolExecutor
    from pathlib import Path
    csrc = Path(__file__).resolve().parent.parent / "sound-event-localization-detection_amd" / "csrc"
    must_not_spill = {"logmel.hip": ("logmel_main_kernel", "logmel_iv_kernel", "stft_kernel"),
                      "spatial.hip": ("gcc_q15_kernel", "gcc_mfma_kernel", "foa_iv_kernel"),
                      # (the bf16 instantiations: what a training iteration runs; the fp32 build of the backward kernel, a
                      #  test yardstick, carries 16 B)
                      "gru.hip": ("gru_forward_kernelI14__hip_bfloat16", "gru_backward_kernelI14__hip_bfloat16")}

    def report(name):
        run = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                              f"-I{csrc.parent.parent / 'include'}", "-Rpass-analysis=kernel-resource-usage", "-c",
                              str(csrc / name), "-o", "/dev/null"], capture_output=True, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        found, current = {}, None
        for line in run.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                current = m.group(1)
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and current:
                found[current] = int(m.group(1))
        return name, found

    with ThreadPoolExecutor(max_workers=3) as pool:
        for name, found in pool.map(report, must_not_spill):
            for kernel in must_not_spill[name]:
                hits = {k: v for k, v in found.items() if kernel in k}
                assert hits, (name, kernel, sorted(found))
                assert all(v == 0 for v in hits.values()), (name, hits)


def test_gcc_table_reproduces_irfft_lags():
    """The constant operand of the matrix-core GCC-PHAT kernel (csrc/spatial.hip, seld_gcc_table_host: fp16 cosine / sine
    fragments) and the way the kernel combines its two products -- cc[+l] = (C[l] + S[l]) / 960, cc[-l] = (C[l] - S[l]) /
    960 -- against numpy's irfft of random unit phase factors; the fragment layout is the one the kernel indexes."""
    import ctypes
    import numpy as np
    import seld_native
    lib = seld_native.load_library()
    halves = np.zeros(2 * 3 * 16 * 64 * 8, dtype=np.uint16)
    assert lib.seld_gcc_table_host(halves.ctypes.data_as(ctypes.c_void_p)) == 0
    frag = halves.view(np.float16).astype(np.float64).reshape(2, 3, 16, 64, 8)      # [part][tile][kstep][lane][j]
    table = np.zeros((2, 48, 512))                                                   # [part][lag][bin]
    for tile in range(3):
        for ks in range(16):
            for lane in range(64):
                table[:, 16 * tile + (lane & 15), 32 * ks + 8 * (lane >> 4):32 * ks + 8 * (lane >> 4) + 8] = \
                    frag[:, tile, ks, lane, :]
    assert not table[:, 33:, :].any() and not table[:, :, 481:].any()               # padding lags / bins are zero
    rng = np.random.default_rng(5)
    phase = np.exp(1j * rng.uniform(-np.pi, np.pi, size=(7, 481)))
    cc = np.fft.irfft(phase, n=960, axis=1)                                          # [7, 960]
    c = phase.real @ table[0, :, :481].T                                             # [7, 48]
    s = phase.imag @ table[1, :, :481].T
    plus = (c + s) / 960.0
    minus = (c - s) / 960.0
    for lag in range(0, 32):
        assert np.abs(plus[:, lag] - cc[:, lag]).max() <= 2e-5
    for lag in range(1, 33):
        assert np.abs(minus[:, lag] - cc[:, 960 - lag]).max() <= 2e-5
    # the kernel's rounding points on top of the table's: the phase factors are formed in fp32 and rounded to fp16 once,
    # products accumulated in fp32.  2000 random rows x 64 lags stay well inside the 1e-4 the GPU tests hold the kernel to.
    phase = np.exp(1j * rng.uniform(-np.pi, np.pi, size=(2000, 481)))
    cc = np.fft.irfft(phase, n=960, axis=1)
    re16 = phase.real.astype(np.float32).astype(np.float16).astype(np.float32)
    im16 = phase.imag.astype(np.float32).astype(np.float16).astype(np.float32)
    c = (re16 @ table[0, :, :481].T.astype(np.float32)).astype(np.float64)
    s = (im16 @ table[1, :, :481].T.astype(np.float32)).astype(np.float64)
    got = np.concatenate([((c - s) / 960.0)[:, 32:0:-1], ((c + s) / 960.0)[:, 0:32]], axis=1)      # lags -32..31
    ref = np.concatenate([cc[:, 928:960], cc[:, 0:32]], axis=1)
    err = np.abs(got - ref)
    assert err.max() <= 6e-5, err.max()
    assert np.sqrt((err ** 2).mean()) <= 1.5e-5


def test_gcc_q15_arithmetic_model():
    """The rounding points of gcc_q15_kernel (csrc/spatial.hip, gq_fragments) restated with numpy on the kernel's own
    table: phasors as Q15 words (round to nearest of 32767 x), the two pair products exact in int32, their UPPER HALF
    after the rounding addend 2^15 (a Q14 integer) converted to fp16, fp32 accumulation, output scale 65536 / 32767^2 /
    960 -- against numpy's irfft of the exact phase factors conj(Um) Un.  Holds the 1e-4 bar of the GPU tests with the
    margin DESIGN.md 7.3 quotes; and why frames with a silent channel (word 0) go another way."""
    import ctypes
    import numpy as np
    import seld_native
    lib = seld_native.load_library()
    halves = np.zeros(2 * 3 * 16 * 64 * 8, dtype=np.uint16)
    assert lib.seld_gcc_table_host(halves.ctypes.data_as(ctypes.c_void_p)) == 0
    frag = halves.view(np.float16).astype(np.float32).reshape(2, 3, 16, 64, 8)
    table = np.zeros((2, 48, 512), dtype=np.float32)
    for tile in range(3):
        for ks in range(16):
            for lane in range(64):
                table[:, 16 * tile + (lane & 15), 32 * ks + 8 * (lane >> 4):32 * ks + 8 * (lane >> 4) + 8] = \
                    frag[:, tile, ks, lane, :]
    rng = np.random.default_rng(11)
    rows = 3000
    um = np.exp(1j * rng.uniform(-np.pi, np.pi, size=(rows, 481)))
    un = np.exp(1j * rng.uniform(-np.pi, np.pi, size=(rows, 481)))
    un[:200] = um[:200] * np.exp(-2j * np.pi * np.arange(481) * 7 / 960)              # a pure delay: R on the unit circle, structured
    q = lambda x: np.clip(np.rint(x * 32767.0), -32767, 32767).astype(np.int64)
    mr, mi, nr, ni = q(um.real), q(um.imag), q(un.real), q(un.imag)
    assert max(np.abs(mr).max(), np.abs(ni).max()) <= 32767
    re, im = mr * nr + mi * ni, mr * ni - mi * nr                                     # v_dot2_i32_i16: exact, |.| < 2^31
    assert np.abs(re).max() < 2 ** 31 and np.abs(im).max() < 2 ** 31
    upper = lambda v: np.floor_divide(v + 32768, 65536)                               # addend 2^15, then bits 31..16 (arithmetic)
    re16 = upper(re).astype(np.float16).astype(np.float32)                            # v_cvt_f16_i16
    im16 = upper(im).astype(np.float16).astype(np.float32)
    c = (re16 @ table[0, :, :481].T).astype(np.float64)
    s_ = (im16 @ table[1, :, :481].T).astype(np.float64)
    scale = 65536.0 / (32767.0 * 32767.0) / 960.0
    got = np.concatenate([((c - s_) * scale)[:, 32:0:-1], ((c + s_) * scale)[:, 0:32]], axis=1)     # lags -32..31
    cc = np.fft.irfft(np.conj(um) * un, n=960, axis=1)
    ref = np.concatenate([cc[:, 928:960], cc[:, 0:32]], axis=1)
    err = np.abs(got - ref)
    assert err.max() <= 7e-5, err.max()
    assert np.sqrt((err ** 2).mean()) <= 1.5e-5
    assert (got[:200].argmax(axis=1) == 32 + 7).all()                                # the planted delay is the peak
    # The factor 1 of a silent channel is NOT representable on that scale -- 32767^2 / 65536 = 16383.0002 is 16384 in fp16,
    # 6.1e-5 too much at lag 0 -- which is why frames with a silent bin take the kernel's exact route (fp32 products, one
    # rounding to fp16, operands in [-1, 1], output scale 1 / 960): there the unit pulse is exact to the table's rounding.
    q14_one = upper(np.full((1, 481), 32767 * 32767, dtype=np.int64)).astype(np.float16).astype(np.float32)
    assert abs(float((q14_one @ table[0, 0, :481]) * scale) - 1.0) > 5e-5
    one = np.ones((1, 481), dtype=np.float16).astype(np.float32)
    c1 = (one @ table[0, :, :481].T).astype(np.float64) / 960.0
    pulse = np.concatenate([c1[:, 32:0:-1], c1[:, 0:32]], axis=1)
    want = np.zeros(64)
    want[32] = 1.0
    assert np.abs(pulse[0] - want).max() <= 1e-5
