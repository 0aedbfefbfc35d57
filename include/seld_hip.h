/* libseld_hip.so -- C ABI of the MI355X (gfx950) SELD hot path.
 *
 * The reference (Zeudon/sound-event-localization-detection) is pure Python on stock PyTorch /
 * torchaudio and has NO FFI of its own; its "plugin surface" is the set of Python names main.py
 * imports.  This header is the boundary a maintainer binds with ctypes
 * (INTEGRATION.md shows the stub): each entry point names the reference call it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, a negative code on failure
 *     (-1 invalid argument, -2 HIP runtime error, -3 seld_init not called, -4 unsupported);
 *     seld_last_error() returns the text of the calling thread's last failure.
 *   - all data pointers are CALLER-OWNED DEVICE pointers (e.g. torch.Tensor.data_ptr());
 *     the library never allocates outputs and never frees inputs.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     all work is asynchronous on it, the library never synchronises.
 *   - int64_t extents; tensors are dense row-major in the layout written next to each pointer.
 *   - one caller thread per device (one process per GPU under torchrun).
 */
#ifndef SELD_HIP_H_
#define SELD_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library state -------------------------------------------------------------------- */
int seld_init(int device);            /* builds the constant tables (Hann, twiddles, sparse mel, GCC cosine / sine) */
int seld_shutdown(void);
int seld_version(void);
const char* seld_last_error(void);

/* The compute-unit count the current device's grids, workspace queries and plans are sized from (>= 1), -3 before
 * seld_init.  It is the device's own count unless the developer switch SELD_CUS=n (an integer >= 1, read once by
 * seld_init; anything else makes seld_init return -1) lowered it to min(n, device count): a test seam that makes every
 * CU-capped kernel walk its grid-stride laps at small shapes, never a tuning knob. */
int seld_num_cus(void);

/* Override the default HTK mel filterbank with a host table fb[481][64] (fp32), e.g. the one
 * torchaudio.functional.melscale_fbanks would build.  Replaces the constant inside
 * torchaudio.transforms.MelScale used at dataset.py:38-43. */
int seld_set_mel_filterbank(const float* fb_host);

/* Override the default (double-precision-rounded) periodic Hann window with a host table w[960],
 * e.g. torch.hann_window(960) as torchaudio.transforms.Spectrogram builds it in fp32. */
int seld_set_window(const float* window_host);

/* Host copies of the default tables -- no GPU needed (used by CPU tests). Any pointer may be NULL. */
int seld_default_tables(float* window960, float* fb481x64, int* mel_b0_64, float* mel_wd_24x64,
                        float* mel_wu_24x64);

/* ---- features: dataset.py:27-58 audio_to_mel_spectrogram ------------------------------ */
/* Number of STFT frames for L samples (center=True, hop 480): 1 + L/480. */
int64_t seld_num_frames(int64_t L);

/* Fused reflect-pad -> frame(960, hop 480) -> periodic Hann -> 960-pt rFFT -> |X|^2 -> HTK mel(64)
 * -> 10*log10(max(.,1e-10)).   pcm [N][C][L] (float in [-1,1), or int16 = float*32768),
 * F = seld_num_frames(L).
 *   layout 0: out [N][C][64][F]   (the reference's [C, n_mels, T] per clip, dataset.py:53)
 *   layout 1: out [N][F][C][64]   (time-major: a training window is a contiguous slice,
 *                                  i.e. the permute(2,0,1) of dataset.py:303 is free)
 * Requires L > 480 (reflect padding), like torch.stft. */
int seld_logmel_f32(const float* pcm, int64_t N, int64_t C, int64_t L, float* out, int layout, void* stream);
int seld_logmel_i16(const int16_t* pcm, int64_t N, int64_t C, int64_t L, float* out, int layout, void* stream);

/* Same kernels with caller-defined output strides (elements): out[n*sN + c*sC + m*sM + t*sT] -- used to write
 * the log-mel channels into a wider time-major feature tensor [N][F][C_total][64] next to the spatial features. */
int seld_logmel_f32_strided(const float* pcm, int64_t N, int64_t C, int64_t L, float* out, int64_t sN, int64_t sC,
                            int64_t sM, int64_t sT, void* stream);
int seld_logmel_i16_strided(const int16_t* pcm, int64_t N, int64_t C, int64_t L, float* out, int64_t sN, int64_t sC,
                            int64_t sM, int64_t sT, void* stream);

/* The strided log-mel pass that ALSO writes the spectra it squares, spec_complex [N][C][F][481] complex64 (what
 * seld_stft_* returns): the spatial features below read them, and one pass over the PCM serves both (north-star
 * additions A14-A16; the reference has no such call -- its STFT lives inside torchaudio, dataset.py:27-58). */
int seld_logmel_spectrum_f32(const float* pcm, int64_t N, int64_t C, int64_t L, float* out, int64_t sN, int64_t sC,
                             int64_t sM, int64_t sT, float* spec_complex, void* stream);
int seld_logmel_spectrum_i16(const int16_t* pcm, int64_t N, int64_t C, int64_t L, float* out, int64_t sN, int64_t sC,
                             int64_t sM, int64_t sT, float* spec_complex, void* stream);

/* The strided log-mel pass that also writes every bin's PHASOR X / |X| as a pair of signed 16-bit fixed-point numbers
 * (word = (re & 0xffff) | im << 16, scale 32767; 0 for a silent bin, |X|^2 <= 1e-12): phasors_q15
 * [N][C][F][seld_phasor_pitch()] words, bins 0..480 of a row written.  This is what GCC-PHAT consumes (seld_gcc_phat_q15):
 * 4 B per bin instead of the 8 B of the complex64 spectrum -- half the HBM bytes between the two kernels -- with the
 * phase transform's reciprocal square root taken once per (channel, bin) where |X|^2 is formed anyway (extends
 * dataset.py:27-58; no upstream counterpart). */
int64_t seld_phasor_pitch(void);
int seld_logmel_phasors_f32(const float* pcm, int64_t N, int64_t C, int64_t L, float* out, int64_t sN, int64_t sC,
                            int64_t sM, int64_t sT, uint32_t* phasors_q15, void* stream);
int seld_logmel_phasors_i16(const int16_t* pcm, int64_t N, int64_t C, int64_t L, float* out, int64_t sN, int64_t sC,
                            int64_t sM, int64_t sT, uint32_t* phasors_q15, void* stream);

/* ---- north-star additions without a reference implementation --------------
 * The reference computes its STFT only implicitly inside torchaudio and has no intensity-vector / GCC-PHAT
 * features; these entry points follow the DCASE SELD-baseline definitions.
 *
 * STFT (the complex spectrum the log-mel kernel squares): out_complex [N][C][F][481] complex64 (interleaved
 * re, im; frame-major).  torch.stft(...) layout is its transpose(-1, -2). */
int seld_stft_f32(const float* pcm, int64_t N, int64_t C, int64_t L, float* out_complex, void* stream);
int seld_stft_i16(const int16_t* pcm, int64_t N, int64_t C, int64_t L, float* out_complex, void* stream);

/* FOA intensity vectors from spectra [N][4][F][481] (channel 0 = W):
 *   I_c[k] = Re(conj(W) X_c) / (1e-8 + |W|^2 + (|X_1|^2+|X_2|^2+|X_3|^2)/3),  iv[c][m] = sum_k fb[k][m] I_c[k]
 * out[n*sN + c*sC + m*sM + t*sT], c = 0..2, m = 0..63. */
int seld_foa_intensity(const float* spec_complex, int64_t N, int64_t F, float* out, int64_t sN, int64_t sC,
                       int64_t sM, int64_t sT, void* stream);

/* The FOA feature set in ONE pass over the PCM (pcm [N][4][L], channel 0 = W): log-mel of the four channels into out
 * channels 0..3 and the three mel-projected intensity vectors (same definition as seld_foa_intensity) into channels 4..6 of
 * out[n*sN + c*sC + m*sM + t*sT]; the spectra stay in LDS.  Extends dataset.py:27-58. */
int seld_logmel_iv_f32(const float* pcm, int64_t N, int64_t L, float* out, int64_t sN, int64_t sC, int64_t sM, int64_t sT,
                       void* stream);
int seld_logmel_iv_i16(const int16_t* pcm, int64_t N, int64_t L, float* out, int64_t sN, int64_t sC, int64_t sM, int64_t sT,
                       void* stream);

/* GCC-PHAT of all C(C-1)/2 channel pairs (m < n, lexicographic) from spectra [N][C][F][481], 2 <= C <= 8:
 *   cc = irfft(R/|R|, 960) with R = conj(X_m) X_n (factor 1 where either channel's bin is silent, |X|^2 <= 1e-12);
 *   out[n*sN + pair*sC + j*sM + t*sT] = cc[(j - 32) mod 960], j = 0..63 (lags -32..31).  With sM == 1 and 16-byte
 *   aligned rows the lags come from the matrix cores (fp16 operands, fp32 accumulation, <= 1e-4 abs vs float64);
 *   any other layout takes the fp32 FFT kernel. */
int seld_gcc_phat(const float* spec_complex, int64_t N, int64_t C, int64_t F, float* out, int64_t sN, int64_t sC,
                  int64_t sM, int64_t sT, void* stream);

/* The same lags from the Q15 phasors of seld_logmel_phasors_* (matrix-core kernel only: unit lag stride, 16-byte aligned
 * rows).  out as for seld_gcc_phat. */
int seld_gcc_phat_q15(const uint32_t* phasors_q15, int64_t N, int64_t C, int64_t F, float* out, int64_t sN, int64_t sC,
                      int64_t sM, int64_t sT, void* stream);

/* Host copy of the matrix-core kernel's constant operand -- no GPU needed (used by the CPU tests): 2 x 3 x 16 fragments of
 * 64 lanes x 8 IEEE binary16 values = 49 152 halves; fragment (part, tile, kstep), lane l, element j holds, for bin
 * k = 32 kstep + 8 (l >> 4) + j and lag n = 16 tile + (l & 15):  part 0: w_k cos(2 pi k n / 960),  part 1: -w_k sin(...),
 * w_0 = w_480 = 1, else 2; zero for k > 480 or n > 32. */
int seld_gcc_table_host(uint16_t* table);

/* ---- mel-band NIPD, the microphone-array cue of FEATURE_SET 'logmel_nipd' (no upstream
 * counterpart).  With P_c[k] the phasor word of channel c, bin k (f_k = 25 k Hz), channel 0 the reference, and the bins IN
 * RANGE those with k >= 1 and min_hz <= f_k <= max_hz:
 *   phi_m[k]  = atan2(Im, Re) of conj(P_0[k]) P_m[k] on the integers of the two words (Re = re0 rem + im0 imm,
 *               Im = re0 imm - im0 rem, exact in int32); 0 when either word is 0 (a silent bin);   m = 1..C-1
 *   nipd_m[j] = sum over in-range k, ascending, in fp32 with fused multiply-adds, of W[k][j] phi_m[k],   j = 0..63
 *   W[k][j]   = fb[k][j] (-sound_speed / (2 pi f_k)) / sum_{k' in range} fb[k'][j],  fb = seld_default_tables' filterbank;
 *               0 for a band without an in-range bin.
 * A channel that is channel 0 delayed by tau seconds has nipd = +sound_speed * tau (metres) in every band.
 *
 * seld_nipd_table_host: W as a sparse table -- host only, no GPU, HOST pointers, any of them may be NULL: band j owns
 * bins first_bin[j] .. first_bin[j] + taps[j] - 1 (taps <= 48: the filterbank's widest band, j = 63, has 44 non-zero bins;
 * 0, and first_bin 0, for an empty band) with the weights w[j * 48 + i] (fp32) / w_f64[j * 48 + i], zero past the band's taps; evaluated in double, summing in ascending k,
 * w = (float) w_f64.  -1 for a range that is negative, reversed, above 12 kHz or holds no bin, or a speed that is not
 * positive.
 *
 * seld_nipd_table_bytes: size of the DEVICE table seld_nipd_q15 reads: int32 first_bin[64], int32 taps[64], float
 * w[64][48], in this order (12 800 bytes).
 *
 * seld_nipd_q15: phasors_q15 [N][C][F][seld_phasor_pitch()] as written by seld_logmel_phasors_*, 2 <= C <= 8;
 *   out[n*sN + (m-1)*sC + j*sM + t*sT] = nipd_m[j] of frame t of clip n;  sM must be 1 and rows 16-byte aligned (out, and
 *   sN, sC, sT multiples of 4), as for seld_gcc_phat_q15.  Only the in-range words of a row are read.  No allocation,
 *   nothing but the kernel on `stream`, with one exception: the FIRST call that sees a table address on a device reads
 *   its 512-byte header back (it synchronises the stream; inside a stream capture that call is refused, so use a table
 *   once before capturing) and refuses a table with a tap count outside 0..48, a band outside bins 1..480 or no taps at
 *   all (-1).  A table's contents must not change while its address is in use; the kernel treats a band it could not
 *   read inside the checked span as empty. */
int seld_nipd_table_host(double min_hz, double max_hz, double sound_speed, int32_t* first_bin, int32_t* taps, float* w,
                         double* w_f64);
int64_t seld_nipd_table_bytes(void);
int seld_nipd_q15(const uint32_t* phasors_q15, int64_t N, int64_t C, int64_t F, const void* table_dev, float* out,
                  int64_t sN, int64_t sC, int64_t sM, int64_t sT, void* stream);

/* ---- labels: dataset.py:60-119 metadata_to_labels + utils.py:77-90 polar_to_grid ---------- */
/* events: int32 [R][5] = (meta_frame, class, source, azimuth_deg, elevation_deg), the CSV rows after
 * the reference's int() casts (dataset.py:93-97).  T = int((L/sr*1000)/20) label frames, computed by
 * the caller with the reference's float64 rule (dataset.py:73).  mask: uint16 [T][I*J], overwritten:
 * bit c set <=> labels[t, cell, c] == 1.0 from an event row; the background one-hot (class 13 where
 * no event, dataset.py:114-117) is implied by mask == 0.  Rows with 5*meta_frame >= T are dropped
 * (empty range in the reference); rows with class outside [0,16) are ignored (the reference raises
 * IndexError for class >= 14 -- the Python host checks that before upload).  I*J must be even. */
int seld_labels_rasterise(const int32_t* events, int64_t R, int64_t T, int I, int J, uint16_t* mask, void* stream);

/* Gaussian-region label augmentation, smrl_seld_gaussian.py:397-534 (active there, absent from the modular
 * dataset.py).  Like seld_labels_rasterise, but every row paints its class into all cells whose centre lies in the
 * +-2 sigma box around centres[r] = (azimuth + az_noise, elevation + el_noise) (float64, degrees; the per-source
 * noise is drawn on the host, :426-437); azimuth wraps, elevation is clipped to [-90, 90]. */
int seld_labels_rasterise_box(const int32_t* events, const double* centres, int64_t R, int64_t T, int I, int J,
                              double sigma_az, double sigma_el, uint16_t* mask, void* stream);

/* mask uint16 [n_cells] -> dense float32 [n_cells][num_classes] exactly as dataset.py:110-117 leaves it. */
int seld_labels_expand(const uint16_t* mask, int64_t n_cells, int num_classes, float* dense, void* stream);

/* ---- windows: dataset.py:267-317 _create_windows ------------------------------------------ */
/* dst[b][w][:] = src[starts[b] + w][:] (rows of row_bytes, a multiple of 16) for rows inside
 * [0, total_rows), zero bytes otherwise: a zero spectrogram pad (dataset.py:293-294) and mask 0 =
 * background for the labels (dataset.py:298-299).  starts: int64 [B] on the device. */
int seld_window_gather(const void* src, int64_t total_rows, int64_t row_bytes, const int64_t* starts, int64_t B,
                       int64_t window, void* dst, void* stream);

/* ---- windows with training augmentation (no upstream counterpart) -------------------------- */
/* The same gather with one transform per window, read from row b of `params`: int32 [B][SELD_AUGMENT_PARAM_INTS] on the
 * device =
 *   [0] spatial pattern p, 0..15, 0 = identity: mirror m = p >> 3 (az -> -az), then k = (p >> 1) & 3 quarter turns
 *       (az -> az + 90 k), then elevation flip e = p & 1 (el -> -el)
 *   [1] [2] time mask 0 (first frame of the window, length)      [3] [4] time mask 1
 *   [5] [6] frequency mask 0 (first of the 64 bins, length)      [7] [8] frequency mask 1
 *   [9] azimuth step r of the rotating gathers further down (these two entry points ignore it)      [10] [11] padding.
 * The kernels reduce p modulo 16 and only compare the mask fields with coordinates they generate themselves: no row can
 * make them read or write out of bounds.  Neither entry point allocates or synchronises (graph-capture safe); a window's
 * output depends on (source, starts[b], params[b]) only. */
#define SELD_AUGMENT_PARAM_INTS 12
#define SELD_AUGMENT_PATTERNS 16
#define SELD_AUGMENT_MAX_CHANNELS 64

/* Features: src float32 [total_rows][channels][64] -> dst float32 [B][window][channels][64],
 *   dst[b][w][c][f] = sign * src[starts[b] + w][source channel of c][f]   (sign flip = XOR of the sign bit: exact),
 * then elements inside a time mask (every channel) or a frequency mask (channels < freq_channels: the log-mel and
 * intensity-vector channels, not GCC-PHAT lags) are set to mask_value.  Rows outside [0, total_rows) stay zero.
 * channel_table: HOST pointer, uint8 [SELD_AUGMENT_PATTERNS][channels], entry = source channel | 0x80 when negated
 * (copied into the kernel's arguments; NULL = every pattern leaves the channels alone). */
int seld_window_gather_augment(const float* src, int64_t total_rows, int channels, int freq_channels, const int64_t* starts,
                               const int32_t* params, int64_t B, int64_t window, const uint8_t* channel_table,
                               float mask_value, float* dst, void* stream);

/* Labels: src uint16 [total_rows][I*J] -> dst uint16 [B][window][I*J], the cell (i, j) of a source row moved to
 *   i' = e ? I-1-i : i,   j' = ((m ? J-1-j : j) + k J/4) mod J;   rows outside [0, total_rows) are zero (background).
 * Labels are never masked.  J % 4 != 0 (a quarter turn is not a whole number of cells) or I*J % 8 != 0: -4. */
int seld_window_permute_mask(const uint16_t* src, int64_t total_rows, int I, int J, const int64_t* starts,
                             const int32_t* params, int64_t B, int64_t window, uint16_t* dst, void* stream);

/* ---- windows with rotation augmentation in azimuth steps (csrc/rotate.hip) ------------------ */
/* Slot [9] of the parameter row above is the azimuth step r (reduced to 0..J-1 by a non-negative modulo; the two entry
 * points above ignore it).  A window's transform: mirror m, then s = (k J/4 + r) mod J cells of azimuth (phi = 2 pi s / J),
 * then elevation flip e, with m, k, e from the pattern.  With c = cos phi, sn = sin phi, sigma = -1 after a mirror else +1:
 *   X' = c X - sn sigma Y,  Y' = sn X + c sigma Y.
 *
 * Rotation terms of a recording, once at construction: spectra [N][4][F][481] complex64 (seld_stft_*, channel 0 = W; ch_x and
 * ch_y in 1..3 name the channels that carry X and Y) ->
 *   out[n*sN + c*sC + m*sM + t*sT], c = 0..2:  P_X = mel |X|^2,  P_Y = mel |Y|^2,  C = mel Re(X conj Y)   (linear fp32),
 * the library's mel filterbank.  No allocation, no synchronisation. */
#define SELD_ROTATE_MAX_STEPS 72
int seld_foa_rotation_terms(const float* spec_complex, int64_t N, int64_t F, int ch_x, int ch_y, float* out, int64_t sN,
                            int64_t sC, int64_t sM, int64_t sT, void* stream);

/* Features: src float32 [total_rows][channels][64] (channels = 4: log-mel W + XYZ in the order ch_x / ch_y / ch_z name;
 * 7: + the three intensity vectors, channel 3 + c pairing W with input channel c) and rot float32 [total_rows][3][64] (the
 * terms above, time-major) -> dst float32 [B][window][channels][64].
 *   4 s % J == 0 (a whole number of quarter turns): bit-identical to seld_window_gather_augment under (m, 4 s / J, e).
 *   otherwise: W and Z log-mel copied, IV_z copied with the flip's sign,
 *     X' log-mel = power_to_db(c^2 P_X + sn^2 P_Y - 2 c sn sigma C),  Y' = power_to_db(sn^2 P_X + c^2 P_Y + 2 c sn sigma C)
 *     (10 log10, floor exactly -100 dB),  IV_x' = c IV_x - sn sigma IV_y,  IV_y' = sn IV_x + c sigma IV_y.
 * (cos, sin) come from a [J][2] fp32 table built here in double precision (exact 0 / +-1 at quarter turns) and passed in the
 * kernel's arguments.  Masks and zero rows as seld_window_gather_augment; channel_table as there, not NULL.
 * J: a multiple of 4, 4..SELD_ROTATE_MAX_STEPS; channels other than 4 and 7: -4. */
int seld_window_gather_rotate(const float* src, const float* rot, int64_t total_rows, int channels, int freq_channels,
                              int ch_x, int ch_y, int ch_z, int J, const int64_t* starts, const int32_t* params, int64_t B,
                              int64_t window, const uint8_t* channel_table, float mask_value, float* dst, void* stream);

/* Labels: seld_window_permute_mask with j' = ((m ? J-1-j : j) + s) mod J. */
int seld_window_permute_mask_rotate(const uint16_t* src, int64_t total_rows, int I, int J, const int64_t* starts,
                                    const int32_t* params, int64_t B, int64_t window, uint16_t* dst, void* stream);

/* ---- per-bin feature standardisation (csrc/standardise.hip and the three gathers) ------------- */
/* Moments of a time-major feature timeline src float32 [total_rows][channels][64]:
 *   moments double [2][channels][64] = (sum over the frames of x, sum over the frames of x * x)   per column (c, f).
 * The summation order is FIXED, so the result is the same bits on every grid, CU count and device (every rank of a
 * data-parallel run computes it from its own copy of the timeline and they agree without a collective):
 *   - the timeline is cut into slabs of SELD_MOMENT_SLAB_FRAMES frames (the last one ragged);
 *   - a slab's partial of a column is the fp64 sum over its frames in ascending order, starting from 0.0;
 *   - the result is the fp64 sum of the slab partials in ascending slab order, starting from 0.0;
 *   - x is widened to fp64 first; the squared term is the fp64 product x * x (exact for an fp32 x), added unfused.
 * A grid-stride kernel writes the slab partials to `workspace` (seld_feature_moments_workspace bytes), a second one folds
 * them; no atomics, no device-scope fence; the timeline is read once.  No allocation, no synchronisation.
 * total_rows <= 0 (there are no statistics of an empty timeline), channels <= 0, a null pointer or a workspace smaller
 * than reported: -1. */
#define SELD_MOMENT_SLAB_FRAMES 1024
int64_t seld_feature_moments_workspace(int64_t total_rows, int channels);   /* bytes; 0 for extents that are refused */
int seld_feature_moments(const float* src, int64_t total_rows, int channels, double* moments, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* The three feature gathers above with one affine map per (OUTPUT channel c, bin f): scale and shift are float32
 * [channels][64] on the device.  With v the fp32 value the gather of the same name without `_affine` writes for an element
 * (after the signed channel copy, or the rotated log-mel / intensity computation), these write
 *   fmaf(v, scale[c][f], shift[c][f])      (one fused multiply-add in fp32),
 * the time and frequency masks are applied AFTERWARDS (a masked element is exactly mask_value) and rows outside
 * [0, total_rows) stay +0.0 over the whole row.  Everything else -- refusals, their order, the parameter rows, graph-capture
 * safety -- as the gather of the same name; scale and shift are refused with the other pointers. */
int seld_window_gather_affine(const float* src, int64_t total_rows, int channels, const int64_t* starts, int64_t B,
                              int64_t window, const float* scale, const float* shift, float* dst, void* stream);
int seld_window_gather_augment_affine(const float* src, int64_t total_rows, int channels, int freq_channels,
                                      const int64_t* starts, const int32_t* params, int64_t B, int64_t window,
                                      const uint8_t* channel_table, float mask_value, const float* scale,
                                      const float* shift, float* dst, void* stream);
int seld_window_gather_rotate_affine(const float* src, const float* rot, int64_t total_rows, int channels, int freq_channels,
                                     int ch_x, int ch_y, int ch_z, int J, const int64_t* starts, const int32_t* params,
                                     int64_t B, int64_t window, const uint8_t* channel_table, float mask_value,
                                     const float* scale, const float* shift, float* dst, void* stream);

/* ---- windows mixed in pairs, labels united (csrc/mix.hip) ------------------------------------ */
/* seld_window_gather_augment(_affine) / seld_window_permute_mask where window b may get a PARTNER: another window of the
 * same timeline.  partners: int64 [B][2] on the device,
 *   partners[b][0] = sb, the partner's start frame;
 *   partners[b][1] = fp32 bits of the linear power gain g in bits 0..31 | the partner's spatial pattern pb in bits 32..35.
 * A g that is not a finite value > 0 (0, negative, NaN, infinity) means NO partner, whatever the other fields hold.  Per
 * output frame w of window b (a = the window itself: start starts[b], pattern and masks of params[b]):
 *   row starts[b] + w outside [0, total_rows):   a zero row;
 *   no partner, or row sb + w outside the timeline:  bit for bit what the entry point without `mix` in its name writes;
 *   otherwise, with x_a / x_b the stored values of the source channels the channel table names for pa / pb:
 *     log-mel channel:     power_to_db(P_a + g P_b),  P = 10^(x/10), P = 0 where x <= -100  (floor exactly -100 dB);
 *     intensity channel:   (E_a IV_a + g E_b IV_b) / (E_a + g E_b), 0 where the denominator is 0,
 *                          E = P_W + (P_X + P_Y + P_Z) / 3 of the operand at that (frame, bin), IV the signed copies;
 *     label cell:          perm_pa(mask[starts[b] + w]) | perm_pb(mask[sb + w]).
 *   Then scale / shift (the _standardised export: the map of the _affine gathers above), then the masks of params[b] on the mixture; labels are never masked.
 * iv_channels: 0 -- every channel is a log-mel channel (any channels <= SELD_AUGMENT_MAX_CHANNELS); 3 with channels == 7 --
 * channels 0..3 log-mel, 4..6 intensity vectors.  Anything else: -4.  The kernels reduce both patterns modulo 16, use sb only
 * through the same row-in-timeline test as starts[b] and only multiply by g: no row of params or partners can make them
 * read or write out of bounds.  No allocation, no synchronisation (graph-capture safe); a window's output depends on
 * (source, starts[b], params[b], partners[b]) only.  Refusals and their order as the entry points they extend. */
int seld_window_gather_mix(const float* src, int64_t total_rows, int channels, int freq_channels, const int64_t* starts,
                           const int32_t* params, const int64_t* partners, int64_t B, int64_t window,
                           const uint8_t* channel_table, float mask_value, int iv_channels, float* dst, void* stream);
int seld_window_gather_mix_standardised(const float* src, int64_t total_rows, int channels, int freq_channels, const int64_t* starts,
                                  const int32_t* params, const int64_t* partners, int64_t B, int64_t window,
                                  const uint8_t* channel_table, float mask_value, int iv_channels, const float* scale,
                                  const float* shift, float* dst, void* stream);
int seld_window_mix_mask(const uint16_t* src, int64_t total_rows, int I, int J, const int64_t* starts, const int32_t* params,
                         const int64_t* partners, int64_t B, int64_t window, uint16_t* dst, void* stream);

/* ---- windows of microphone-array features under a channel swap (csrc/micswap.hip) ---------- */
/* seld_window_gather_augment(_affine) for the feature sets of a microphone array whose geometry is known.  A spatial pattern
 * that maps the array onto itself permutes the microphones: the transformed scene's channel j is the recording's channel
 * sigma_p(j).  mic_perm: HOST pointer, int8 [SELD_AUGMENT_PATTERNS][mics], row p = sigma_p, or all -1 when pattern p is no
 * symmetry of the array (a window with such a pattern is written with the identity transform).  Row 0 is the identity.
 * src float32 [total_rows][channels][64] -> dst float32 [B][window][channels][64], per output channel, sigma = sigma_p:
 *   log-mel c < mics:  the stored channel sigma(c), copied.
 *   SELD_MIC_GCC  (channels = mics + mics (mics - 1) / 2; pairs lexicographic, lags -32..31 at indices 0..63, as seld_gcc_phat):
 *     pair (a, b), a < b, with u = sigma(a), v = sigma(b):  u < v: the stored pair (u, v), copied;  u > v: the stored pair
 *     (v, u) with the lags reversed, out[j] = in[64 - j] for j = 1..63 and out[0] = in[0] (lag +32 is not stored: the -32
 *     slot of a reversed pair keeps the stored -32 value, the one element that is not the transformed field's).
 *   SELD_MIC_NIPD (channels = 2 mics - 1; channel mics + m - 1 = NIPD of microphone m = 1..mics-1 against microphone 0):
 *     N(sigma(m)) - N(sigma(0)), one fp32 subtraction, N(0) = +0.0f, N(i) the stored NIPD of microphone i; a plain copy when
 *     sigma(0) = 0.  Exact for phase differences that do not wrap, an approximation where they do.
 * Then scale / shift (the _standardised export, the map of the _affine gathers above: fmaf(v, scale[c][f], shift[c][f]),
 * both float32 [channels][64] on the device), then the masks of params[b] as seld_window_gather_augment; rows outside
 * [0, total_rows) are +0.0.  The operations go to the kernel by value; it reduces the pattern modulo 16 and only compares
 * the mask fields: no row can make it read or write out of bounds.  No allocation, no synchronisation (graph-capture
 * safe); a window's output depends on (source, starts[b], params[b]) only.  Refused, in this order and before anything is
 * written: mics outside 2..8, an unknown kind, freq_channels outside 0..channels (-1, with the other extents); a mic_perm
 * row that is neither a permutation nor all -1, a row 0 that is not the identity (-1); a window too large (-4); null
 * pointers (-1). */
#define SELD_MIC_GCC 0
#define SELD_MIC_NIPD 1
int seld_window_gather_mic(const float* src, int64_t total_rows, int mics, int kind, int freq_channels, const int64_t* starts,
                           const int32_t* params, int64_t B, int64_t window, const int8_t* mic_perm, float mask_value,
                           float* dst, void* stream);
int seld_window_gather_mic_standardised(const float* src, int64_t total_rows, int mics, int kind, int freq_channels,
                                  const int64_t* starts, const int32_t* params, int64_t B, int64_t window,
                                  const int8_t* mic_perm, float mask_value, const float* scale, const float* shift,
                                  float* dst, void* stream);

/* ---- frequency shift, gain curve and cutouts in place on a gathered batch (csrc/spectral.hip) -- */
/* One stage for all the feature gathers above: batch float32 [B][window][channels][64], as any of them wrote it WITHOUT masks
 * and WITHOUT scale / shift, is rewritten in place.  spectral: int32 [B][SELD_SPECTRAL_PARAM_INTS] on the device =
 *   [0] frequency shift s in bins (signed)      [1] flags, bit 0: this window has a gain curve
 *   [2] [3] [4] [5] cutout 0 (first frame, frames, first bin, bins)      [6] [7] [8] [9] cutout 1      [10] [11] padding.
 * curves: float32 [B][64] on the device (dB per destination bin), or NULL: no window has a curve.  params: the parameter
 * rows of the gathers above (only their mask fields [1..8] are read), or NULL: no masks.  Per window b, frame w, channel c,
 * bin f, in this order:
 *   1. row starts[b] + w outside [0, total_rows): the row is left as the gather wrote it (zeros);
 *   2. c < freq_channels:  v = batch[b][w][c][clamp(f - s, 0, 63)]  (edge replication; an exact copy), else v = batch[b][w][c][f];
 *   3. c < logmel_channels and the window has a curve:  v <= -100 (power_to_db's floor: power 0) stays, else
 *      v = max(v + curves[b][f], -100)  (one fp32 addition);
 *   4. the _standardised export:  v = fmaf(v, scale[c][f], shift[c][f]), the map of the _affine gathers above;
 *   5. the time / frequency masks of params[b] as seld_window_gather_augment, then the two cutouts: an element with w in
 *      [t, t + tl), f in [f0, f0 + fl) and c < freq_channels becomes mask_value.  A masked element is exactly mask_value.
 * With s = 0, no curve and no cutout the result is bit for bit what the gather's own masking / standardising export writes.
 * A window with s = 0, no curve, no cutout and no mask is not touched by the export without scale / shift.
 * In place and race-free: every lane loads only the 16 bytes it stores; shifted bins move between the 16 lanes of a 256-byte
 * row in registers.  The shift only selects a bin through the clamp, cutouts and masks are only compared, a curve value is
 * only added, starts only pass the row-in-timeline test: no row can move a load or a store out of the batch.  No allocation,
 * no synchronisation (graph-capture safe).  Refused: the extents, channels <= 0 or not 0 <= logmel_channels <= freq_channels
 * <= channels (-1); a window too large (-4); B == 0 returns 0 before any pointer is looked at; batch, starts, spectral (and
 * scale, shift) null (-1). */
#define SELD_SPECTRAL_PARAM_INTS 12
int seld_window_spectral(float* batch, int64_t total_rows, int channels, int logmel_channels, int freq_channels,
                         const int64_t* starts, const int32_t* params, const int32_t* spectral, const float* curves,
                         int64_t B, int64_t window, float mask_value, void* stream);
int seld_window_spectral_standardised(float* batch, int64_t total_rows, int channels, int logmel_channels, int freq_channels,
                                      const int64_t* starts, const int32_t* params, const int32_t* spectral,
                                      const float* curves, int64_t B, int64_t window, float mask_value, const float* scale,
                                      const float* shift, void* stream);

/* ---- per-channel energy normalisation of the log-mel channels (csrc/pcen.hip) ------------------- */
/* x float32 [N][T][C_total][64], time-major: n the clip, t the frame, c the channel, f the mel bin.  The first C_log channels
 * are log-mel in dB as the feature kernels above write them.  For every clip, every c < C_log and every f:
 *   E[t] = 2^(x[t] log2(10) / 10)                    the stored value back as mel power: the -100 dB floor is 1e-10
 *   M[t] = a M[t-1] + s E[t],  a = 1 - s,  M[-1] = E[0]     (the steady-state start; the smoother starts afresh in every clip)
 *   y[t] = (E[t] (eps + M[t])^-alpha + delta)^r - delta^r
 * and out[n][t][c][f] = y[t].  s comes from a time constant tau in seconds at 50 frames per second: T_f = 50 tau,
 * s = (sqrt(1 + 4 T_f^2) - 1) / (2 T_f^2), computed in float64 by the caller and passed as one float.  Channels c >= C_log
 * (intensity vectors, GCC lags, NIPD) are neither read nor written.  out has x's layout; out == x (in place) is allowed,
 * any other overlap is refused; with out != x, out's channels c >= C_log are left untouched.
 *
 * The arithmetic is FIXED, so the result is the same bits on every grid, CU count and device, a clip's result does not depend
 * on the other clips of the call, and frame t does not depend on frames after it or on T:
 *   - fp32 throughout; u^v is exp2(fl(v log2(u))) with the hardware's exp2 / log2 (v_exp_f32, v_log_f32);
 *     E = exp2(fl(x c)), c = fl32(log2(10) / 10); a = fl(1 - s);
 *   - the time axis is cut into chunks of SELD_PCEN_CHUNK_FRAMES frames anchored at a clip's frame 0 (the last one ragged);
 *   - the aggregate of a chunk k that has a successor is A_k = the state after its 256 frames from state 0,
 *     M <- fmaf(a, M, fl(s E)) in ascending frame order;
 *   - the state entering chunk k is Horner over the earlier chunks in ascending order from E[0]:
 *     M <- fmaf(a256, M, A_j), j = 0 .. k - 1, a256 = fl32(a^256 evaluated in double);
 *   - inside the chunk M <- fmaf(a, M, fl(s E)), then y = fl(exp2(fl(r log2(fl(fl(E g) + delta)))) - dr) with
 *     g = exp2(fl(-alpha log2(fl(eps + M)))) and dr = fl32(delta^r evaluated in double); nothing else is fused.
 * Two launches on `stream`: the first writes E[0] and the aggregates to `workspace` (seld_pcen_workspace bytes: float
 * [N][chunks][C_log][64], row 0 of a clip E[0], row 1 + k the aggregate A_k), the second reads its own chunk's frames of x
 * and the workspace, nothing else -- so in place no workgroup reads what another may have overwritten.  No spin, no
 * look-back, no atomics, no device-scope fence, no allocation, no synchronisation.
 * -1: a null pointer; N < 1 or T < 1; C_log < 1 or C_log > C_total; a non-finite parameter; s outside (0, 1]; alpha outside
 * [0, 1]; r outside (0, 1]; delta <= 0 or eps <= 0; a workspace smaller than reported; out overlapping x without being x.
 * -4: extents beyond the kernels' 32-bit chunk indices; a pointer that is not 16-byte aligned. */
#define SELD_PCEN_CHUNK_FRAMES 256
int64_t seld_pcen_workspace(int64_t N, int64_t T, int C_total, int C_log);   /* bytes; 0 for extents that are refused */
int seld_pcen(const float* x, float* out, int64_t N, int64_t T, int C_total, int C_log, float s, float alpha, float delta,
              float r, float eps, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- loss: loss.py:43-54 class_mse_loss (+ its backward) ---------------------------------- */
/* logits [n_cells][14] (fp32, or bf16 when logits_is_bf16), labels as EITHER the compact mask
 * (uint16 [n_cells]) OR dense float32 [n_cells][14] (exactly one non-NULL).  Writes
 * loss_out[0] = mean((softmax(logits) - y)^2) and, if grad != NULL, grad (same dtype/shape as logits)
 * = grad_scale * p_k * ((p_k - y_k) - sum_c p_c (p_c - y_c)); pass grad_scale = 2*w/(n_cells*14) for
 * d(w*loss)/dlogits.  workspace: seld_softmax_mse_workspace_bytes() bytes of device scratch.
 * Deterministic (fixed-order reduction, no float atomics).
 * Alignment: logits and grad may be any pointer aligned for their element type.  Full 256-cell tiles move in 16-byte
 * pieces when the pointer (logits for the load, grad for the store) is 16-byte aligned, element by element otherwise;
 * the result is the same bits either way.  Dense label rows are read as float2 (8-byte aligned). */
int64_t seld_softmax_mse_workspace_bytes(void);
int seld_softmax_mse(const void* logits, int logits_is_bf16, const uint16_t* mask, const float* dense_labels,
                     int64_t n_cells, int num_classes, float grad_scale, float* loss_out, void* grad,
                     void* workspace, void* stream);

/* ---- loss: loss.py:27-41 class_ce_loss (+ its backward), optional focal factor (csrc/loss_ce.hip) ---- */
/* logits and labels as seld_softmax_mse, alignment included.  The target t of a cell is the first maximal dense label
 * (torch.argmax) or, for a mask m, the lowest set bit of m & 0x3fff, background (13) if there is none.  class_weights: 14 fp32
 * on the DEVICE, or NULL for all ones.  With p = softmax(z), q = sum_{c != t} p_c, W = sum_cells w_t:
 *   out[0] = (1/W) sum_cells w_t q^gamma (-log p_t)      out[1] = W
 *   grad   = grad_scale (w_t / W) f (p_k - [k = t]),  f = q^gamma - gamma p_t q^(gamma-1) log p_t   (if grad != NULL)
 * focal_gamma = 0 is nn.CrossEntropyLoss(weight = class_weights) and runs a kernel without the focal arithmetic; otherwise
 * focal_gamma >= 1 (finite).  A cell with q == 0 contributes nothing.  The host never reads W: four launches, capturable,
 * deterministic (integer class counts, fixed-order double sums, no global atomics).
 * workspace: seld_softmax_ce_workspace_bytes() bytes of device scratch.
 * -4: num_classes != 14, n_cells * 14 at or above the limit of seld_softmax_mse; -1: n_cells <= 0, a NULL logits / out /
 * workspace, both or neither of mask / dense_labels, focal_gamma negative, non-finite or in (0, 1). */
int64_t seld_softmax_ce_workspace_bytes(void);
int seld_softmax_ce(const void* logits, int logits_is_bf16, const uint16_t* mask, const float* dense_labels,
                    int64_t n_cells, int num_classes, const float* class_weights, float focal_gamma, float grad_scale,
                    float* out, void* grad, void* workspace, void* stream);

/* data[0..n) *= *scale with the scale read from DEVICE memory (the upstream gradient autograd hands the loss):
 * when it is exactly 1.0 -- what loss.backward() passes -- every block returns after one load and the data is not
 * touched.  n must be a multiple of 8; data bf16 when is_bf16, else fp32, 16-byte aligned. */
int seld_scale_by_device_scalar(void* data, int is_bf16, int64_t n, const float* scale, void* stream);

/* The optimiser step of trainer.py:112-116,179 (torch.optim.Adam with weight_decay as L2 added to the gradient; amsgrad off)
 * for a LIST of tensors in one launch per 48 tensors, arithmetic of the framework's fused kernel in fp32:
 *   g = grad * grad_scale + weight_decay * p;  m += (1 - beta1)(g - m);  v = beta2 v + (1 - beta2) g g;
 *   p -= (lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * grad[k]: bf16 when grad_is_bf16[k] (the gradient of a bf16 working weight: no separate cast), else fp32; param / exp_avg /
 * exp_avg_sq fp32; low_bf16[k]: the bf16 working copy rewritten from the new master, or NULL.  All tensors of an entry
 * share one memory layout (the kernel walks the storage).  lr and step are DEVICE scalars (step = the count of THIS
 * update, i.e. already incremented, a whole number).  beta1 / beta2 are doubles: 1 - beta and 1 - beta^step are formed in
 * double and rounded to fp32 once, as the framework does.  HOST arrays of device addresses / lengths, passed to the kernel
 * by value. */
int seld_multi_adam(const void* const* grad, const int32_t* grad_is_bf16, float* const* param, float* const* exp_avg,
                    float* const* exp_avg_sq, void* const* low_bf16, const int64_t* lengths, int count, const float* lr,
                    const float* step, double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                    void* stream);

/* ---- guarded update: global gradient-norm clipping, non-finite step skip, weight EMA (csrc/guard.hip, csrc/adam.hip) ----
 * The device-side record the norm pass writes and the guarded Adam reads: 8 words, 32 bytes, 16-byte aligned, zeroed by
 * the caller once before the first call (the two counters are cumulative).  The flags are floats so that framework ops can
 * use them as they are (`skipped` is what torch's fused Adam takes as found_inf). */
typedef struct seld_guard_record {
  float grad_norm;        /* sqrt(sum over all tensors of (g * grad_scale)^2); inf / NaN when an element is not finite */
  float clip_coef;        /* min(1, max_norm / (grad_norm + 1e-6)) evaluated in fp32; exactly 1.0f when max_norm <= 0 */
  float apply;            /* 1.0f: update; 0.0f: skip (only when grad_norm is not finite AND skip_nonfinite was set) */
  float skipped;          /* 1.0f - apply */
  int32_t steps_skipped;  /* cumulative: calls that ended with apply == 0 */
  int32_t steps_clipped;  /* cumulative: applied calls with clip_coef < 1 */
  int32_t reserved[2];
} seld_guard_record;

/* Global L2 norm of a LIST of gradient tensors and the guard record, one launch per 48 tensors plus one single-workgroup
 * launch, deterministic (fixed-order sums, no atomics): pass 1 writes one fp32 partial per 4096-element chunk of every
 * tensor (at most 25 fp32 additions per partial), pass 2 sums the partials in double.  grad / grad_is_bf16 / lengths as
 * for seld_multi_adam (HOST arrays; tensors walked as storage).  partial: device scratch of at least
 * *partial_floats = seld_multi_grad_norm_scratch(lengths, count) floats, rewritten by every call.  A finite gradient
 * whose squares overflow fp32 inside one chunk (|g * grad_scale| above ~1e17) reads as non-finite. */
int seld_multi_grad_norm_scratch(const int64_t* lengths, int count, int64_t* partial_floats);
int seld_multi_grad_norm(const void* const* grad, const int32_t* grad_is_bf16, const int64_t* lengths, int count,
                         float grad_scale, float max_norm, int skip_nonfinite, float* partial, int64_t partial_floats,
                         seld_guard_record* guard, void* stream);

/* seld_multi_adam with a guard: every workgroup returns before its first store when guard->apply == 0 (param, exp_avg,
 * exp_avg_sq, the bf16 working copies and ema untouched); otherwise the gradient is grad * grad_scale * guard->clip_coef
 * (in that order: a coefficient of exactly 1 gives seld_multi_adam's bits; weight decay is added after clipping) and, where
 * ema[k] != NULL and ema_decay != 0, ema[k] += (1 - ema_decay) * (p_new - ema[k]) from the fp32 value just computed (fp32,
 * the master's layout) in the same pass.  ema == NULL: no EMA at all; guard == NULL: always apply, coefficient 1.  The
 * caller advances `step` only for applied updates (e.g. step += 1 before the call, step -= guard->skipped after it). */
int seld_multi_adam_guarded(const void* const* grad, const int32_t* grad_is_bf16, float* const* param,
                            float* const* exp_avg, float* const* exp_avg_sq, void* const* low_bf16, const int64_t* lengths,
                            int count, const float* lr, const float* step, double beta1, double beta2, float eps,
                            float weight_decay, float grad_scale, float* const* ema, float ema_decay,
                            const seld_guard_record* guard, void* stream);

/* One launch per 96 tensors casts a list of tensors (the fp32-master / bf16-working-weight mode of the trainer):
 * src / dst are HOST arrays of `count` device addresses, lengths a HOST array of element counts (the descriptors are
 * passed to the kernel by value).  bf16_to_fp32 != 0: bf16 sources -> fp32 destinations (gradients); 0: fp32 -> bf16
 * (weights), round to nearest even.  Source and destination of a pair must share their memory layout (the cast walks
 * the storage).  No reference counterpart: replaces the per-parameter casts of torch.autocast. */
int seld_multi_cast(const void* const* src, void* const* dst, const int64_t* lengths, int count, int bf16_to_fp32,
                    void* stream);

/* LayerNorm over the last dimension [-> ReLU], activations in their own dtype (csrc/layernorm.hip).  Replaces the
 * head's nn.LayerNorm(512) -> nn.ReLU of model_crnn.py:77-83 (model_conformer.py / resnet50_model.py: LayerNorm(1024)).
 * x, y, dy, dx [rows][D] contiguous, fp32 or bf16 (is_bf16); weight, bias [D] fp32; statistics and arithmetic in fp32
 * (biased two-pass variance, eps inside the square root: torch.nn.functional.layer_norm).  D in {256, 512, 1024, 2048}
 * (seld_layernorm_supported).  forward writes mean_rstd [rows][2] fp32 -- with x, all the backward pass needs (the
 * ReLU mask is recomputed).  backward writes dx, dweight [D], dbias [D] (fp32, deterministic two-level sums);
 * workspace: seld_layernorm_workspace_floats(rows, D) floats. */
int seld_layernorm_supported(int64_t D);
int64_t seld_layernorm_workspace_floats(int64_t rows, int64_t D);
int seld_layernorm_forward(const void* x, int is_bf16, int64_t rows, int64_t D, const float* weight, const float* bias,
                           float eps, int relu, void* y, float* mean_rstd, void* stream);
int seld_layernorm_backward(const void* x, const void* dy, int is_bf16, int64_t rows, int64_t D, const float* weight,
                            const float* bias, const float* mean_rstd, int relu, void* dx, float* dweight,
                            float* dbias, float* workspace, void* stream);

/* Hold `stream` for `nanoseconds` (0 .. 1e6) with a one-wavefront kernel that watches the 100 MHz wall clock.
 * Used at the head of the side stream that carries weight-gradient GEMMs beside a BiGRU recurrence
 * (seld_gru_backward): the recurrence's 16 workgroups each need a whole CU's LDS and must be resident before the
 * GEMMs occupy every CU.  No upstream counterpart (the reference's trainer.py:165-179 is single-stream). */
int seld_stream_delay(int64_t nanoseconds, void* stream);

/* The three-term SMR-SELD loss of smrl_seld_gaussian.py:946-1072 (loss.py:43-54, 56-146 on probabilities), value and
 * gradient in one pass (csrc/loss3.hip):  total = w_class * MSE(softmax(logits), y) + w_aiur * AIUR + w_cl * CL.
 * logits [frames][rows*cols][14] fp32 or bf16; labels as seld_softmax_mse (uint16 mask per cell, or dense fp32);
 * rows x cols = the I x J DOA grid (18 x 36), at least 3 x 3 and at most 1024 cells.  loss_out4 (device) receives
 * (total, mse, aiur, cl).  grad (nullable, dtype of logits) = d total / d logits for an upstream gradient of 1 (the AIUR
 * term is argmax based and has none).  workspace: seld_smr_loss_workspace_bytes(frames, rows * cols) bytes.
 * Deterministic (fixed-order double partial sums, integer event counts). */
int64_t seld_smr_loss_workspace_bytes(int64_t frames, int64_t cells_per_frame);
int seld_smr_loss(const void* logits, int logits_is_bf16, const uint16_t* mask, const float* dense_labels,
                  int64_t frames, int rows, int cols, int num_classes, float w_class, float w_aiur, float w_cl,
                  float* loss_out4, void* grad, void* workspace, void* stream);

/* ---- glue kernels of the training iteration (csrc/glue.hip): each replaces a chain of 3-10 framework launches of a
 * few microseconds (clone / fill / add / cast, fill + reduce + copy, slice copies, flip + copy) by one launch ---- */

/* nn.GRU's biases (model_crnn.py:65-72) as the recurrence consumes them: gi_bias [2][3][H] (bf16 when out_is_bf16,
 * else fp32) = b_ih + (r, z rows of b_hh), the bias of the input-projection GEMM; b_hn [2][H] fp32 = n rows of b_hh.
 * b_ih, b_hh: [2][3H] fp32 (forward, reverse). */
int seld_gru_fold_bias(const float* b_ih, const float* b_hh, int64_t H, void* gi_bias, int out_is_bf16, float* b_hn,
                       void* stream);

/* seld_gru_fold_bias and, in the same launch, the parameter-only operand of the backward recurrence: w_hh_t_bf16
 * [2][H][3H] bf16 = W_hh ([2][3H][H], fp32 or bf16 when w_is_bf16) rounded to bf16 (nearest even) and transposed per
 * direction -- what seld_gru_backward / seld_gru_backward_direct take as w_hh_t.  H must be a multiple of 32. */
int seld_gru_prepare(const float* b_ih, const float* b_hh, const void* w_hh, int w_is_bf16, int64_t H, void* gi_bias,
                     int out_is_bf16, float* b_hn, void* w_hh_t_bf16, void* stream);

/* seld_gru_backward's per-tile bias sums `partial` [tiles][2][4][H] -> nn.GRU's bias gradients db_ih [2][3H] =
 * (da_r, da_z, da_n) and db_hh [2][3H] = (da_r, da_z, da_n r), fp32, tiles added in a fixed order. */
int seld_gru_bias_grads(const float* partial, int64_t tiles, int64_t H, float* db_ih, float* db_hh, void* stream);

/* out[i] = sum over c of partial[c][i], i < count (fp32 accumulation, fixed order): the reduction behind a split-K
 * weight-gradient product (the autograd dW = dY^T X of every nn.Linear, trainer.py:178).  partial [chunks][count] bf16
 * or fp32, out [count] bf16 or fp32. */
int seld_sum_chunks(const void* partial, int in_is_bf16, int64_t chunks, int64_t count, void* out, int out_is_bf16,
                    void* stream);

/* seld_sum_chunks with the columns re-ordered on the way out: partial [chunks][rows][F][C], out [rows][C][F],
 * out[row][c * F + f] = sum over chunks of partial[chunk][row][f * C + c].  The same accumulation per element (fp32,
 * chunks in order, one rounding), so the result equals seld_sum_chunks followed by the column permutation bit for bit.
 * dW_ih of the first GRU layer, whose input features are ordered (frequency, channel) while the parameter's columns are
 * (channel, frequency) (model_crnn.py:114-116).  F in 2..4, C % 8 == 0, 16-byte aligned tensors. */
int seld_sum_chunks_columns(const void* partial, int in_is_bf16, int64_t chunks, int64_t rows, int64_t C, int64_t F,
                            void* out, int out_is_bf16, void* stream);

/* out[n] = sum over r of g[r][n]: the bias gradient of an nn.Linear (autograd for trainer.py:178) from the [rows][n_cols]
 * output gradient, bf16 or fp32, n_cols % 8 == 0, 16-byte aligned.  Two launches: row blocks summed in parallel into
 * `partial` [seld_column_sums_blocks(rows, n_cols)][n_cols] fp32 (caller-owned), then added in a fixed order. */
int64_t seld_column_sums_blocks(int64_t rows, int64_t n_cols);
int seld_column_sums(const void* g, int in_is_bf16, int64_t rows, int64_t n_cols, float* partial, void* out, int out_is_bf16,
                     void* stream);

/* Multi-tensor forms of the two reductions above, for a backward pass that queues them (every nn.Linear of
 * model_conformer.py:19-41,98-127 / resnet50_model.py:80-91 contributes one of each; nothing reads a weight or bias
 * gradient before the optimiser of trainer.py:179): ONE launch per 64 chunk sums, TWO (row-block partials, fixed-order
 * finish) per 40 column sums, descriptors by value.  flags[k]: bit 0 = the input is bf16, bit 1 = the output is bf16.
 * seld_multi_column_sums needs caller-owned fp32 scratch `partial` sized by seld_multi_column_sums_scratch. */
int seld_multi_sum_chunks(const void* const* partial, void* const* out, const int64_t* counts, const int32_t* chunks,
                          const int32_t* flags, int count, void* stream);
int seld_multi_column_sums_scratch(const int64_t* rows, const int64_t* n_cols, int count, int64_t* partial_floats);
int seld_multi_column_sums(const void* const* g, void* const* out, const int64_t* rows, const int64_t* n_cols,
                           const int32_t* flags, int count, float* partial, int64_t partial_floats, void* stream);

/* dW_hh [2][3H][H] of nn.GRU from the two chunked products the host forms over both directions at once:
 * p_gi [chunks][2][3][H][2][H] = (da_r, da_z, da_n)^T h_prev, p_n [chunks][2][H][2][H] = (da_n r)^T h_prev; the blocks
 * with matching directions (and, of p_gi, the r and z gates) are summed over the chunks and written in place. */
int seld_gru_dwhh_finish(const void* p_gi, const void* p_n, int in_is_bf16, int64_t chunks, int64_t H, void* dw_hh,
                         int out_is_bf16, void* stream);

/* wt[i][o][2-r][2-s] = w[o][i][r][s] for 3x3 weights, both in channels-last memory (w: [O][3][3][I], wt: [I][3][3][O]):
 * the weights with which the DATA gradient of a 3x3 / stride 1 / pad 1 convolution (model_crnn.py:5-17) is itself a
 * forward convolution.  elem_bytes 2 (bf16) or 4. */
int seld_conv_weight_flip_transpose(const void* w, int elem_bytes, int64_t O, int64_t I, void* wt, void* stream);

/* Weight gradient of a 3x3 / stride 1 / pad 1 / bias-free convolution (model_crnn.py:5-17) on channels-last bf16
 * tensors: x [B][T][F][Cin] (the saved input), dy [B][T][F][Cout] -> dw [Cout][3][3][Cin] (the weight's channels-last
 * memory), bf16 when dw_is_bf16, else fp32.  F in {8, 16, 32}, Cin % 64 == 0, Cout % 64 == 0 (see _supported); all
 * pointers 16-byte aligned.  Split over K slabs that each write an fp32 partial into `workspace`
 * (seld_conv3x3_wgrad_workspace_floats floats, no initialisation needed), added in a fixed order by a second launch:
 * deterministic, no atomics. */
int seld_conv3x3_wgrad_supported(int64_t F, int64_t Cin, int64_t Cout);
int64_t seld_conv3x3_wgrad_workspace_floats(int64_t B, int64_t T, int64_t F, int64_t Cin, int64_t Cout);
int seld_conv3x3_wgrad(const void* x, const void* dy, int64_t B, int64_t T, int64_t F, int64_t Cin, int64_t Cout,
                       void* dw, int dw_is_bf16, float* workspace, void* stream);

/* Data gradient of the same convolution from the weights where they lie (csrc/convdgrad.hip): dy [B][T][F][Cout] and
 * w [Cout][3][3][Cin] (the weight's channels-last memory) -> dx [B][T][F][Cin], all bf16, fp32 accumulation, one
 * rounding.  dx[b][t][f][ci] = sum over (r, s, co) of dy[b][t+1-r][f+1-s][co] * w[co][r][s][ci]: no flipped, transposed
 * copy of the weights is formed.  F in {8, 16, 32}, Cin % 64 == 0, Cout % 64 == 0 (see _supported); all pointers
 * 16-byte aligned.  Every output is written once in a fixed summation order: deterministic, no atomics, no workspace. */
int seld_conv3x3_dgrad_supported(int64_t F, int64_t Cin, int64_t Cout);
int seld_conv3x3_dgrad(const void* dy, const void* w, int64_t B, int64_t T, int64_t F, int64_t Cin, int64_t Cout,
                       void* dx, void* stream);

/* Forward of the same convolution on the data-gradient kernel's loop (csrc/convfwd.hip): x [B][T][F][Cin] and
 * w [Cout][3][3][Cin] -> y [B][T][F][Cout], all bf16, fp32 accumulation, one rounding; the weights are read as they
 * lie.  F in {8, 16, 32}, Cin % 64 == 0, Cout % 64 == 0 (see _supported); all pointers 16-byte aligned.
 * partials (may be NULL): [2][chunks][Cout] fp32 with chunks = seld_conv3x3_forward_chunks(B, T, F); row c receives the
 * sum and the sum of squares per output channel of the bf16 values stored for chunk c (256 positions of one clip, fewer
 * in a clip's last chunk), summed in a fixed order: the input of seld_conv_tail_forward_from_partials. */
int seld_conv3x3_forward_supported(int64_t F, int64_t Cin, int64_t Cout);
int64_t seld_conv3x3_forward_chunks(int64_t B, int64_t T, int64_t F);
int seld_conv3x3_forward(const void* x, const void* w, int64_t B, int64_t T, int64_t F, int64_t Cin, int64_t Cout,
                         void* y, float* partials, void* stream);

/* ---- First encoder block with the convolution recomputed in place (csrc/convfirst.hip) --------------------- */
/* Conv3x3(4 -> 64, stride 1, pad 1, no bias) -> BatchNorm2d (training mode, affine, running statistics) -> ReLU ->
 * MaxPool2d((1,2)) of model_crnn.py:5-17 without ever writing the convolution output or its gradient.
 *   in  [B][T][F][4] bf16 (channels-last memory of the [B, 4, T, F] input; it needs no gradient), 8-byte aligned
 *   w   [64][4][3][3] bf16 (w_is_bf16) or fp32 (rounded to bf16 as autocast would) with element strides
 *       w_sco, w_sci, w_sr, w_ss (output channel, input channel, kernel row, kernel column)
 *   F in {16, 32, 64, 128, 256} (see _supported)
 * forward : y [B][T][F/2][64] bf16; mean_invstd [2][64], scale_shift [2][64] fp32 (kept for backward); the running
 *   statistics are updated like nn.BatchNorm2d.  Same expressions and roundings as seld_conv_tail_forward on the
 *   bf16 convolution output (fp32 accumulation, one rounding).
 * backward: from dy [B][T][F/2][64] bf16: dw (the convolution's weight gradient, bf16 when dw_is_bf16 else fp32, written
 *   with element strides dw_s*), dgamma [64], dbeta [64] fp32.
 * workspace: seld_convfirst_workspace_floats(backward) floats, no initialisation needed.  phases: 3 in normal use;
 *   1 launches only the first kernel (statistics / reduction), 2 only what follows it (finalise + apply / finalise +
 *   weight gradient + sum), for timing.
 * Deterministic: no atomics, every sum in a fixed order. */
int seld_convfirst_supported(int64_t F, int64_t Cin, int64_t Cout);
int64_t seld_convfirst_workspace_floats(int backward);
int seld_convfirst_forward(const void* in, const void* w, int w_is_bf16, int64_t w_sco, int64_t w_sci, int64_t w_sr,
                           int64_t w_ss, int64_t B, int64_t T, int64_t F, const float* bn_weight, const float* bn_bias,
                           float* running_mean, float* running_var, float momentum, float eps, void* y,
                           float* mean_invstd, float* scale_shift, float* workspace, int phases, void* stream);
int seld_convfirst_backward(const void* in, const void* w, int w_is_bf16, int64_t w_sco, int64_t w_sci, int64_t w_sr,
                            int64_t w_ss, const void* dy, int64_t B, int64_t T, int64_t F, const float* mean_invstd,
                            const float* scale_shift, void* dw, int dw_is_bf16, int64_t dw_sco, int64_t dw_sci,
                            int64_t dw_sr, int64_t dw_ss, float* dgamma, float* dbeta, float* workspace, int phases,
                            void* stream);

/* ---- CNN block tail: BatchNorm2d -> ReLU -> MaxPool2d((1,2)) at model_crnn.py:5-17 (ConvBlock.forward) ---- */
/* x: the convolution output in channels-last memory order = row-major [rows = B*T*F][C] (bf16 when is_bf16, else
 * fp32); the two frequency bins of a pooling pair are adjacent rows.  pool = 2: MaxPool2d((1,2)); pool = 1: no
 * pooling; pool = 4: no pooling and SiLU instead of ReLU (BatchNorm1d -> Swish of the Conformer convolution module,
 * model_conformer.py:71-96, rows = B*T).  C must be 8 * (a divisor of 256); rows even when pool = 2.
 * forward, training != 0: batch statistics (biased variance), running_mean / running_var updated with `momentum`
 *   (unbiased variance) exactly like nn.BatchNorm2d; training == 0: the running statistics are used.
 *   y [rows/pool][C] (dtype of x) = max over the pair of relu(weight * (x - mean) * invstd + bias), with the
 *   BatchNorm output rounded to the activation dtype before the comparisons like the unfused modules.
 *   mean_invstd [2][C], scale_shift [2][C] (a = weight*invstd, b = bias - mean*a): outputs, kept for backward.
 * backward: dx [rows][C] (dtype of x), dweight [C], dbias [C] from dy [rows/pool][C]; the ReLU mask and pooling
 *   argmax are recomputed from x (first element wins ties, as max_pool2d).
 * workspace: seld_conv_tail_workspace_floats(C) floats of device scratch.  Deterministic (no float atomics). */
int64_t seld_conv_tail_workspace_floats(int C);
int seld_conv_tail_forward(const void* x, const void* residual, int is_bf16, int64_t rows, int C, int pool,
                           const float* weight, const float* bias, float* running_mean, float* running_var,
                           float momentum, float eps, int training, void* y, float* mean_invstd, float* scale_shift,
                           float* workspace, void* stream);
/* The training-mode forward without its statistics pass: partials [2][nrows][C] holds plain (unshifted) sums of x and
 * x^2 over disjoint parts of the rows (seld_conv3x3_forward), 1 <= nrows <= seld_conv_tail_partial_rows(); they are
 * combined in double in a fixed order.  No residual. */
int64_t seld_conv_tail_partial_rows(void);
int seld_conv_tail_forward_from_partials(const void* x, int is_bf16, int64_t rows, int C, int pool,
                                         const float* partials, int64_t nrows, const float* weight, const float* bias,
                                         float* running_mean, float* running_var, float momentum, float eps, void* y,
                                         float* mean_invstd, float* scale_shift, void* stream);
int seld_conv_tail_backward(const void* x, const void* residual, const void* dy, int is_bf16, int64_t rows, int C,
                            int pool, const float* mean_invstd, const float* scale_shift, void* dx, void* dresidual,
                            float* dweight, float* dbias, float* workspace, void* stream);

/* ---- Conformer convolution module: depthwise Conv1d over time, model_conformer.py:71-96 ------------------- */
/* nn.Conv1d(D, D, K, padding=(K-1)/2, groups=D) evaluated in the channels-last layout of the surrounding layers:
 * x, y [B][T][D] (bf16 when is_bf16, else fp32), weight [D][K] fp32, bias [D] fp32 or NULL, odd K <= 31, D % 64 == 0.
 * flip_taps != 0 evaluates the data gradient (dx from dy with the taps reversed; pass bias = NULL).
 * seld_dwconv1d_wgrad: partial [R][D][32] fp32 with R = seld_dwconv1d_wgrad_rows(B, T) (one row per batch row and
 * 50-step time chunk) -- slots 0..K-1 = sum_t dy[t] x[t + k - pad] over the chunk, slot 31 = sum_t dy[t]; the caller adds
 * the rows (dweight = partial.sum(0)[:, :K], dbias = partial.sum(0)[:, 31]). */
int seld_dwconv1d(const void* x, int is_bf16, const float* weight, const float* bias, int64_t B, int64_t T, int D, int K,
                  int flip_taps, void* y, void* stream);
int64_t seld_dwconv1d_wgrad_rows(int64_t B, int64_t T);
int seld_dwconv1d_wgrad(const void* x, const void* dy, int is_bf16, int64_t B, int64_t T, int D, int K, float* partial,
                        void* stream);

/* ---- recurrence: nn.GRU(2048, 256, num_layers=2, bidirectional) at model_crnn.py:65-72 ------- */
/* One bidirectional GRU layer's recurrence, all T steps in one launch (both directions), H = 256.
 * The batch is processed in tiles of S = seld_gru_tile_rows() sequences (2 in this build; tiles = ceil(B / S)):
 * one workgroup per (tile, direction); the other columns of each 16-column MFMA are padding so that the
 * per-CU vector-memory and gate-math work of a step -- what bounds it once the weights are resident -- is
 * spread over more CUs.
 *
 * Streamed per-step tensors use the kernels' private TILE LAYOUT so that every wavefront load / store
 * is one contiguous run: with P = 16/S lanes sharing a sequence and U = 8/P units per lane, a tensor
 * X[b][t][dir][slot][u] (b = S*tile + seq, u = 32*w + 16*s + 4*q + i, 4*s + i = U*part + j) is stored as
 * [tile][t][dir][w(8)][slot(NS)][q(4)][part(P)][seq(S)][j(U)]  (seld_gru_to_tile / seld_gru_from_pair_tile
 * convert; seld_native.to_tile / from_tile are their torch definitions).
 *   gi         [B][T][2][3][H] NATURAL layout -- the input GEMM's output as it is (no permute: the loads are 4 bytes
 *                    per lane either way): x W_ih^T + b_ih, gates r|z|n, direction 0 = forward in time,
 *                    1 = reverse (fp32, or bf16 when is_bf16).  The recurrent biases of the r and z gates
 *                    (b_hh[0:2H]) must ALREADY be added in (they commute with the sigmoid argument).
 *   w_hh       [2][3H][H] bf16;   b_hn [2][H] fp32 (= b_hh[2H:3H] per direction);   h0 = 0
 *   y          [tiles*S][T][2H] natural layout (h_t; forward direction in [..., :H]), dtype of gi; rows >= B are
 *                    scratch of the last tile's padding sequences (which re-read sequence B-1's gi)
 *   saved_tile       r, z, n, (W_hn h + b_hn) per step for the backward pass, or NULL: 2 pair-slots (r|z, n|gh_n),
 *                    i.e. [tile][t][dir][w(8)][2][lane(64)][2][U]; fp32 when gi is fp32, IEEE fp16 when is_bf16
 *                    (O(1) values: 8x finer than bf16 at half of fp32's bytes -- the recurrence is bound by one
 *                    CU's load/store path).  Opaque to the caller: tiles*T*2*8*2*64*2*U elements.
 * MFMA bf16 operands, fp32 accumulation, fp32 gates and state. */
int64_t seld_gru_tile_rows(void);
int seld_gru_forward(const void* gi, int is_bf16, const void* w_hh_bf16, const float* b_hn, int64_t B,
                     int64_t T, int64_t H, void* y, void* saved_tile, void* stream);

/* Backward of the recurrence.  dy_tile NS=1 (dtype of y), y = the forward output (all tiles*S rows),
 * w_hh_t [2][H][3H] bf16 (W_hh transposed).
 * dg_tile (dtype of y): da_r, da_z, da_n, da_n*r as 2 pair-slots (da_r|da_z, da_n|da_n*r), i.e.
 * [tile][t][dir][w(8)][2][q(4)][part(P)][seq(S)][2][j(U)] -- the first three are d/d(gi); (da_r, da_z, da_n*r) are
 * d/d(gh), from which the caller forms dW_hh = dgh^T h_prev and with gi's GEMM dW_ih, dx.
 * dbias [tiles][2][4][H] fp32: the four slots summed over the tile's sequences and all t (add the tiles for
 * db_ih = slots (0,1,2) and db_hh = slots (0,1,3)). */
int seld_gru_backward(const void* dy_tile, const void* saved_tile, const void* y, int is_bf16,
                      const void* w_hh_t_bf16, int64_t tiles, int64_t T, int64_t H, void* dg_tile, float* dbias,
                      void* stream);

/* The same backward recurrence on the caller's own layouts (bf16 and 4-sequence tiles only: kErrUnsupported otherwise): dy and y
 * natural [B][T][2H] with exactly B rows (the last tile's padding sequences re-read row B-1 and contribute exact
 * zeros), dgi [B][T][2][3][H] = (da_r, da_z, da_n) and dghn [B][T][2][H] = da_n*r written contiguously, rows >= B never
 * touched; saved_tile, w_hh_t and dbias ([ceil(B/S)][2][4][H]) as above.  Bit-identical to seld_gru_to_tile ->
 * seld_gru_backward -> seld_gru_from_pair_tile, without the two converter launches. */
int seld_gru_backward_direct(const void* dy, const void* saved_tile, const void* y, int is_bf16,
                             const void* w_hh_t_bf16, int64_t B, int64_t T, int64_t H, void* dgi, void* dghn,
                             float* dbias, void* stream);

/* Layout converters for seld_gru_backward (HBM-bound permutes; elem_bytes = 2 for bf16, 4 for fp32).
 * seld_gru_to_tile: natural src [B][T][2][ns][H] -> tile layout dst (B padded with zeros to whole tiles).
 * seld_gru_from_pair_tile: the backward kernel's dg_tile -> dgi [B][T][2][3][H] (da_r, da_z, da_n) and
 * dghn [B][T][2][H] (da_n*r), both contiguous -- what the caller's GEMMs read. */
int seld_gru_to_tile(const void* src, int elem_bytes, int64_t B, int64_t T, int ns, void* dst, void* stream);
int seld_gru_from_pair_tile(const void* dg_tile, int elem_bytes, int64_t B, int64_t T, void* dgi, void* dghn,
                            void* stream);

/* h_{t-1} of the forward recurrence, natural layout: y [B][T][2][H] (the forward output, h_t) ->
 * h_prev[b][t][0] = y[b][t-1][0], h_prev[b][t][1] = y[b][t+1][1], zero at each direction's first step.  The operand of
 * the recurrent weight gradient dW_hh = sum_t dgh_t^T h_{t-1} (what autograd through model_crnn.py:65-72's nn.GRU
 * accumulates step by step). */
int seld_gru_previous_state(const void* y, int elem_bytes, int64_t B, int64_t T, void* h_prev, void* stream);

/* ---- evaluation: spatial grid maps -> DOA events, location-aware matching (csrc/seld_eval.hip) -----------------
 * No reference counterpart (its test_model, trainer.py:394-711, reports argmax accuracy per cell); the definitions are
 * this project's, DESIGN.md section 10.  Grid 18 x 36 (cell = i*36 + j), 14 classes (13 = background), windows of 250
 * frames with hop 50 over a timeline of `total` frames: W = ceil(total / 50) windows, window w starts at frame 50 w.
 *
 * seld_grid_decode: logits [nw][250][648][14] (bf16 when is_bf16, else fp32; 16-byte aligned) hold windows
 * [w0, w0+nw).  meta_first int64 / meta_len int32 [Q] (device) give the first global frame and the frame count (1..5)
 * of every meta-frame of the timeline.  Meta-frames [q0, q0+nq) are decoded:
 *   P_q[cell][c] = mean over the frames f of q (ascending) of the mean over the windows covering f (ascending w) of
 *   softmax(logits[w][f - 50 w][cell][:])[c], fp32;  a detection is a cell whose P_q >= threshold and that beats its
 *   8 neighbours (azimuth wraps, no wrap over the poles; equal scores: the lower cell wins), the first K (1..8) of them
 *   by (score descending, cell ascending).
 * Outputs, row qi = q - q0:  det_cell int32 [nq][13][K] (-1 past the count), det_score f32 [nq][13][K] (0 past the
 * count), det_count int32 [nq][13]; probs_out f32 [nq][648][13] = P_q, or NULL.  One workgroup per meta-frame, fixed
 * summation order: bit-identical however the meta-frames are split across calls.
 * Every window that covers a requested meta-frame must be in the call: the check needs the tables' values, so the
 * host does it on its own copy (seld_native.grid_decode raises before launching); the kernel itself writes nothing
 * for a meta-frame whose windows are not all present. */
int seld_grid_decode(const void* logits, int is_bf16, int64_t w0, int64_t nw, int64_t W, int64_t total,
                     const int64_t* meta_first, const int32_t* meta_len, int64_t q0, int64_t nq, float threshold, int K,
                     int32_t* det_cell, float* det_score, int32_t* det_count, float* probs_out, void* stream);

/* seld_doa_match: one thread per (q, c) of nq meta-frames x 13 classes.  Detections as seld_grid_decode writes them
 * (det_cell [nq][13][K], det_count [nq][13]; DOA = the cell centre az = -180 + (j + 1/2) 360/J,
 * el = -90 + (i + 1/2) 180/I); references: CSR ref_offsets int32 [nq*13 + 1] over ref_dirs int32 [R][2] = (azimuth,
 * elevation) degrees, at most 8 per (q, c) (the host checks).  With d the float64 great-circle angle in degrees:
 *   stats int32 [nq][13][4] = (R, P, k = min(R, P), tp = size of a maximum matching among pairs with d <= thr_deg),
 *   cost f64 [nq][13] = minimum total d over injective assignments of size k (0 when k = 0). */
int seld_doa_match(const int32_t* det_cell, const int32_t* det_count, int K, const int32_t* ref_offsets,
                   const int32_t* ref_dirs, int64_t nq, int I, int J, double thr_deg, int32_t* stats, double* cost,
                   void* stream);

/* ---- test-time augmentation of the decode (csrc/seld_tta.hip) ------------------------------
 * seld_grid_decode_tta: seld_grid_decode over n_patterns (1..16) transformed copies of the windows, averaged in the
 * ORIGINAL frame before the peak test.  logits [n_patterns][nw][250][648][14], contiguous: stack n holds windows
 * [w0, w0+nw) gathered with spatial pattern patterns[n] (0..15, no duplicates; SELD_AUGMENT_* below seld_window_gather:
 * mirror p >> 3, then (p >> 1) & 3 quarter turns, then elevation flip p & 1), so that an event at original cell (i, j)
 * shows in stack n at dest_n(i, j) = (e ? 17 - i : i, ((m ? 35 - j : j) + 9 k) mod 36).  `patterns` is a HOST pointer,
 * read before the launch (the list travels by value in the kernel arguments: no upload, graph-capture safe).
 *   p_f[cell][c] = (sum over the windows w covering frame f (ascending), inside it over n (ascending), of
 *                   softmax(logits[n][w][f - 50 w][dest_n(cell)][:])[c]) / (n_w * n_patterns), fp32
 *   P_q = mean of p_f over the frames of q (ascending), and everything after it, as seld_grid_decode.
 * patterns = {0} gives seld_grid_decode's outputs bit for bit.  Outputs, the coverage rule (a meta-frame whose windows
 * are not all present writes nothing; the host checks before launching), no allocation, no synchronise: as
 * seld_grid_decode.  -1 for n_patterns outside 1..16, a pattern outside 0..15, a duplicate, K outside 1..8, null
 * pointers. */
int seld_grid_decode_tta(const void* logits, int is_bf16, int64_t w0, int64_t nw, int64_t W, int64_t total,
                         const int64_t* meta_first, const int32_t* meta_len, int64_t q0, int64_t nq,
                         const int32_t* patterns, int n_patterns, float threshold, int K, int32_t* det_cell,
                         float* det_score, int32_t* det_count, float* probs_out, void* stream);

/* ---- track linking of the decoded detections (csrc/seld_track.hip) ---------------------------
 * seld_track_link: detections as seld_grid_decode writes them (det_cell [Q][13][K], det_count [Q][13]; a count above K is
 * K, a cell outside [0, I*J) ends its list) -> event tracks.  A chain is one (segment s, class c), x = 13 s + c, its
 * frames m = 0..M_s-1 at q = seg_offsets[s] + m (seg_offsets int64 [S+1], device), walked in ascending m; chains are
 * independent.  dist(a, b) = dist_table[i_a][i_b][(j_b - j_a) mod J] (int32 [I][I][J], device, I*I*J <= 16384):
 * milli-degrees between the cell centres, built by the host.  Per chain 8 slots, free or (id, cell, first_m, last_m),
 * next_id = 0.  At frame m with detections d_0..d_{n-1} in rank order:
 *   1. a slot with m - last_m > max_gap + 1 becomes free;
 *   2. candidates: (occupied slot t, rank r) with dist(slot.cell, d_r) <= gate_mdeg, taken in ascending (dist, t, r)
 *      when neither t nor r has been taken this frame: emit (id, slot.cell) at every frame last_m+1..m-1 (the fill),
 *      then slot.cell = d_r, last_m = m, emit (id, d_r) at m;
 *   3. each unlinked detection in rank order takes the lowest free slot, else the slot not linked this frame with the
 *      smallest last_m (lowest index on ties; that track ends): id = next_id++, first_m = last_m = m, emit (id, d_r).
 * A track with last_m - first_m + 1 < min_len is removed, fills included.  Outputs: trk_cell / trk_id int32 [Q][13][8]
 * = the surviving emissions of (q, c) in ascending id, -1 past trk_count int32 [Q][13]; tracks int32 [T][4] =
 * (first_m, last_m, detected frames, kept), track id of chain x at row chain_offsets[x] + id (chain_offsets int64
 * [13 S + 1], device: the exclusive prefix sum of the chains' detection counts, an upper bound on their tracks; rows no
 * track uses are not written); chain_tracks int32 [13 S] = next_id.  trk_cell, trk_id and tracks 16-byte aligned.
 * Two launches (the chain walk, one wavefront per chain; filter and compaction, one thread per (q, c)), integer
 * arithmetic, plain stores in a fixed order: exact and independent of the schedule.  No allocation, no synchronise.
 * -1, launching nothing, for K outside 1..8, max_gap outside 0..16, min_len < 1, gate_mdeg < 0 or a null pointer. */
int seld_track_link(const int32_t* det_cell, const int32_t* det_count, int K, const int64_t* seg_offsets, int64_t S,
                    const int32_t* dist_table, int I, int J, int gate_mdeg, int max_gap, int min_len,
                    const int64_t* chain_offsets, int32_t* trk_cell, int32_t* trk_id, int32_t* trk_count, int32_t* tracks,
                    int32_t* chain_tracks, void* stream);

/* ---- sub-cell DOA refinement of the decode (csrc/seld_refine.hip) ----------------------------
 * seld_grid_decode_refine: seld_grid_decode (n_patterns == 0 and patterns == NULL: the plain walk over logits
 * [nw][250][648][14]) or seld_grid_decode_tta (n_patterns 1..16: logits [n_patterns][nw][250][648][14], `patterns` a HOST
 * pointer) with one more output.  det_cell, det_score, det_count and probs_out are what that export writes for the same
 * input, bit for bit.  For the detection of class c at peak cell x = (i, j), with N(x) = x and its up-to-8 neighbours
 * under the peak test's rule (j +- 1 mod 36; i +- 1 only inside [0, 18)) and u(y) = cell_unit[y] (f32 [648][3], device:
 * the unit vector (cos el cos az, cos el sin az, sin el) of the centre of cell y, computed in float64 by the host and
 * rounded once):
 *   v = sum over y in N(x) of P_q[y][c] u(y), fp32 fused multiply-adds in the order di = -1, 0, 1 outer, dj = -1, 0, 1
 *   inner (the centre included);  az = atan2(v_y, v_x), el = atan2(v_z, hypot(v_x, v_y)) in degrees, az = +180 written
 *   as -180;  the cell centre when |v|^2 is 0 or not finite.
 * det_dir f32 [nq][13][K][2] = (az, el) of detection r of (qi, c), 0 past the count; 16-byte aligned.  An epilogue of
 * the decode while P_q is in LDS: no extra pass over memory, no second launch; one workgroup per meta-frame, plain
 * stores in a fixed order: bit-identical however the meta-frames are split across calls.  Coverage rule, no
 * allocation, no synchronise: as seld_grid_decode.  -1, launching nothing, for what seld_grid_decode_tta refuses
 * (n_patterns 0 allowed, exactly when patterns is NULL), and for a null cell_unit or det_dir. */
int seld_grid_decode_refine(const void* logits, int is_bf16, int64_t w0, int64_t nw, int64_t W, int64_t total,
                            const int64_t* meta_first, const int32_t* meta_len, int64_t q0, int64_t nq,
                            const int32_t* patterns, int n_patterns, float threshold, int K, const float* cell_unit,
                            int32_t* det_cell, float* det_score, int32_t* det_count, float* det_dir, float* probs_out,
                            void* stream);

/* seld_doa_match_dirs: seld_doa_match with the detections' directions given as det_dir f32 [nq][13][K][2] = (azimuth,
 * elevation) degrees (what seld_grid_decode_refine writes; 8-byte aligned) in place of det_cell, I, J.  The directions
 * are widened to float64; distance, matching and assignment are seld_doa_match's own code, so the exact cell centres
 * reproduce its stats and cost bit for bit. */
int seld_doa_match_dirs(const float* det_dir, const int32_t* det_count, int K, const int32_t* ref_offsets,
                        const int32_t* ref_dirs, int64_t nq, double thr_deg, int32_t* stats, double* cost, void* stream);

/* ---- threshold sweep of the evaluation (csrc/seld_sweep.hip) --------------------------------------
 * The detections of a (q, c) are sorted by (score descending, cell ascending) and the peak test does not depend on the
 * threshold, so the list at any threshold t >= t0 is a prefix of the list decoded at t0.
 *
 * seld_doa_match_prefix: seld_doa_match (det_dir NULL: det_cell, I, J name the detections) or seld_doa_match_dirs (det_dir
 * f32 [nq][13][K][2], 8-byte aligned, in place of det_cell, I, J) for every prefix of every (q, c) in one launch:
 *   ptp int32 [nq][13][K+1], pcost f64 [nq][13][K+1]: entry p <= min(det_count, K) = the tp and the cost that export
 *   writes when the entry's count is replaced by p (tp equal, cost bit-equal); entries past the count repeat the entry at
 *   the count.  An entry seld_doa_match refuses (more than 8 references, a count outside 0..K) is -1 / NaN throughout.
 * One thread per (q, c); no allocation, no synchronise.  -1, launching nothing, for K outside 1..8, bad extents or a null
 * pointer. */
int seld_doa_match_prefix(const int32_t* det_cell, const float* det_dir, const int32_t* det_count, int K,
                          const int32_t* ref_offsets, const int32_t* ref_dirs, int64_t nq, int I, int J, double thr_deg,
                          int32_t* ptp, double* pcost, void* stream);

/* seld_sweep_score: the sums behind the metrics at T thresholds from the prefix tables.  `thresholds` is a HOST pointer to T
 * floats (1 <= T <= 64, strictly ascending, in (0, 1]; else -1), read before the launch and passed by value in the kernel
 * arguments.  With R = ref_offsets[qc+1] - ref_offsets[qc], P_t = the number of LEADING detections of (q, c) with
 * det_score >= thresholds[t] (fp32, the decode's comparison; det_score f32 [nq][13][K], det_count clamped to 0..K),
 * k = min(R, P_t), tp = ptp[qc][P_t] (a refused entry: k = tp = -1) and chunk x = meta-frames [x chunk, min(nq, (x+1) chunk)):
 *   counts int64 [T][n_chunks][13][5] = per class the sums of (tp, P_t - tp, R - tp, R, k) over the chunk,
 *   sdi    int64 [T][n_chunks][3]     = sums over the chunk's meta-frames of (min(FN_q, FP_q), max(0, FN_q - FP_q),
 *                                       max(0, FP_q - FN_q)), FN_q / FP_q summed over the 13 classes of q,
 *   cost   f64   [T][n_chunks][13]    = per class the sum of pcost[qc][P_t] in ascending q,
 * n_chunks = ceil(nq / chunk), chunk >= 1.  One lane per threshold, one wave per chunk, plain stores: a repeated run is
 * bit-identical.  No allocation, no synchronise. */
int seld_sweep_score(const int32_t* ptp, const double* pcost, const float* det_score, const int32_t* det_count, int K,
                     const int32_t* ref_offsets, int64_t nq, const float* thresholds, int T, int64_t chunk,
                     int64_t* counts, int64_t* sdi, double* cost, void* stream);

/* ---- segment-based, class-macro metrics with jackknife replicates (csrc/seld_segment.hip) ---------
 * No reference counterpart; the definitions are DESIGN.md section 18.1 (after the DCASE 2022/23 segment-based metric).
 *
 * seld_doa_assign: the minimum-cost assignment of seld_doa_match (det_dir NULL: det_cell, I, J name the detections) or
 * seld_doa_match_dirs (det_dir f32 [nq][13][K][2], 8-byte aligned, in place of det_cell, I, J) itself, not only its cost.
 * Rows are the smaller side (the references when R <= P), k = rows; the dp runs over the sets of used columns in ascending
 * mask order, the row of a mask being popcount - 1: dp[mask] = the minimum over its set bits b, ascending, strict <, of
 * dp[mask ^ bit b] + d[row][b], choice[mask] = the b that set it; the final mask is the first of popcount k whose dp is
 * strictly smallest; the pairs are read back through choice.  The distances and additions are seld_doa_match's in its
 * order, so the assigned distances, added in row order, are its cost bit for bit.
 *   pair_dist f64 [nq][13][8]: slot r = the distance in degrees of reference r (its position in the CSR list of (q, c)) to
 *   the detection assigned to it; NaN when reference r is unassigned or r >= R, and throughout for an entry seld_doa_match
 *   refuses (more than 8 references, a count outside 0..K).
 * thr_deg does not enter the assignment (it is checked, >= 0, and otherwise unused: the argument list is
 * seld_doa_match_prefix's).  One thread per (q, c); no allocation, no synchronise.  -1, launching nothing, for K outside
 * 1..8, bad extents or a null pointer. */
int seld_doa_assign(const int32_t* det_cell, const float* det_dir, const int32_t* det_count, int K,
                    const int32_t* ref_offsets, const int32_t* ref_dirs, int64_t nq, int I, int J, double thr_deg,
                    double* pair_dist, void* stream);

/* seld_segment_score: the counts of every (1 s block, class) from pair_dist, then every recording's blocks folded.
 * Recording s holds meta-frames seg_offsets[s] .. seg_offsets[s+1] - 1 (int64 [S+1], device); its block x covers its
 * meta-frames 10 x .. min(10 x + 10, M_s) - 1 and is row block_offsets[s] + x (int64 [S+1], device: the exclusive prefix
 * sum of ceil(M_s / 10); NB = block_offsets[S]).  Per (block, class), over the block's frames in ascending order with
 * R_m = the references and P_m = det_count clamped to 0..K:  nref = max R_m, npred = max P_m;  in a frame with R_m > 0 and
 * P_m > 0 every non-NaN slot r adds its distance to sum_r and 1 to cnt_r;  a slot with cnt_r > 0, in ascending r:
 * avg = sum_r / cnt_r, de += avg, DE_TP += 1, TP += 1 when avg <= thr_deg else FPs += 1.  Then
 *   nref > 0 and npred > 0, some slot matched:  FP = max(0, npred - nref), FN = max(0, nref - npred)
 *   nref > 0 and npred > 0, no slot matched:    FN = nref, FP = npred
 *   npred = 0: FN = nref;  nref = 0: FP = npred;  DE_FN = FN throughout.
 *   seg_stats  int32 [NB][13][8]  = (nref, npred, TP, FPs, FP, FN, DE_TP, DE_FN),  seg_de f64 [NB][13] = de
 *   rec_counts int64 [S][13][11]  = the eight summed over the recording's blocks, then S_c, D_c, I_c = the sums of
 *                                   min(locFP, locFN), max(0, locFN - locFP), max(0, locFP - locFN) with
 *                                   locFP = FPs + FP and locFN = FN of the (block, class)
 *   rec_sdi    int64 [S][3]       = the same three terms with locFP / locFN summed over the block's 13 classes first
 *   rec_de     f64   [S][13]      = seg_de summed over the recording's blocks in ascending order
 * Two launches, one workgroup per recording each; plain stores in a fixed order: a repeated run is bit-identical.  No
 * allocation, no synchronise.  -1, launching nothing, for K outside 1..8, S < 0, thr_deg < 0 or a null pointer. */
int seld_segment_score(const double* pair_dist, const int32_t* det_count, int K, const int32_t* ref_offsets,
                       const int64_t* seg_offsets, const int64_t* block_offsets, int64_t S, double thr_deg,
                       int32_t* seg_stats, double* seg_de, int64_t* rec_counts, int64_t* rec_sdi, double* rec_de,
                       void* stream);

/* seld_jackknife_score: the metrics of every leave-one-recording-out replicate.  Replicate j = 0..S-1 sums rec_counts,
 * rec_sdi and rec_de over every recording but j, replicate S over all of them; recordings in ascending order, per class.
 * From a set of counts:  F = TP / (TP + FPs + (FP + FN) / 2),  ER = (S + D + I) / Nref,  LE = de / DE_TP (180 when
 * DE_TP = 0),  LR = DE_TP / (DE_TP + DE_FN),  SELD = (ER + (1 - F) + LE / 180 + (1 - LR)) / 4;  an empty denominator is NaN.
 *   out f64 [S+1][2][5]: row 0 micro = the figures of the counts summed over the classes (de: the class sums added in
 *   ascending class order) with rec_sdi's S, D, I; row 1 macro = each figure's plain mean, in ascending class order, over
 *   the classes with Nref > 0 in that replicate, from the class's own counts and S_c, D_c, I_c (NaN when there is none).
 *   out_class f64 [13][5]: the per-class figures of replicate S.
 * One lane per replicate; no allocation, no synchronise.  -1, launching nothing, for S < 1 or a null pointer. */
int seld_jackknife_score(const int64_t* rec_counts, const int64_t* rec_sdi, const double* rec_de, int64_t S, double* out,
                         double* out_class, void* stream);

/* ---- sample-rate conversion in front of the 24 kHz feature kernels (csrc/resample.hip) ---------
 * No reference counterpart (dataset.py:27-58 hands the file's rate to MelSpectrogram).  A windowed-sinc polyphase FIR with
 * zero delay and zero extension: with g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g,
 *   y[m] = sum over t of x[q - (t - half)] * table[p][t],  p = (m * down) mod up,  q = (m * down) div up,  x = 0 outside
 *   [0, L),  m = 0 .. L_out - 1,  L_out = ceil(L * up / down);  output sample m sits at time m / rate_out.
 *
 * seld_resample_plan: the geometry of the designed table for a pair of rates -- host only, no GPU.  Any pointer may be
 * NULL.  -1, with the rate and the limit in seld_last_error(), for a rate that is not positive or needs up > 320 phases
 * or more than 1100 taps per output (8000, 11025, 12000, 16000, 22050, 32000, 44100, 48000, 88200, 96000 and 192000 Hz
 * to 24000 Hz pass).
 *
 * seld_resample_table_host: the designed table itself -- host only, no GPU, HOST pointers: table [up][taps] fp32 and / or
 * table_f64 [up][taps] (either may be NULL), table = (float) table_f64.  table[p][t] = g[p + (t - half) * up] of the
 * prototype on the dense grid fs = rate_in * up: Kaiser window (beta 10.06) over 64 zero crossings per side of a sinc
 * with cut-off 0.95 * min(rate_in, rate_out) / 2, gain up, evaluated in double. */
int seld_resample_plan(int64_t rate_in, int64_t rate_out, int* up, int* down, int* taps, int* half);
int seld_resample_table_host(int64_t rate_in, int64_t rate_out, float* table, double* table_f64);

/* The conversion.  pcm [N][C][L] (float, or int16 scaled by 2^-15 on load like seld_logmel_i16), table_dev [up][taps]
 * fp32 on the DEVICE (the caller uploads what seld_resample_table_host wrote, or a table of its own: taps must be
 * 2 * half + 1, 1 <= up, down <= 32768, half <= 32768), out [N][C][L_out] fp32 with L_out = ceil(L * up / down) exactly (-1 otherwise).
 * fp32 accumulation with fused multiply-adds, one output written once: deterministic, and a (clip, channel) row does not
 * depend on the others of the call.  64-bit sample indices.  No allocation, no synchronise, no state inside the library:
 * the call needs no seld_init.  -4 when `down` is so large that the input span of one output does not fit 64 KB of LDS
 * (no designed table is). */
int seld_resample_f32(const float* pcm, int64_t N, int64_t C, int64_t L, const float* table_dev, int up, int down, int taps,
                      int half, float* out, int64_t L_out, void* stream);
int seld_resample_i16(const int16_t* pcm, int64_t N, int64_t C, int64_t L, const float* table_dev, int up, int down, int taps,
                      int half, float* out, int64_t L_out, void* stream);

/* ---- per-window class statistics for class-balanced window sampling (csrc/balance.hip) ---------
 * No reference counterpart (main.py:60-74 shuffles uniformly).  mask is the label timeline of seld_labels_rasterise laid
 * end to end: uint16 [total_rows][cells], bit c of a word = class c active in that cell.  Integer work: both results are
 * the same bits on every grid and device.  No allocation, no synchronisation, no atomics.
 *
 * seld_frame_class_mask:  frame_mask[t] = bitwise OR over the `cells` words of row t, t = 0 .. total_rows - 1.  The
 * timeline is read once, in 16-byte chunks: mask 16-byte aligned and cells a multiple of 8 (at most 2048), else -4; a
 * timeline too long for 32-bit row indices: -4.  A null pointer, total_rows < 1 or cells < 1: -1.
 *
 * seld_window_class_frames:  counts int32 [n_windows][SELD_BALANCE_COLUMNS]; window w covers the frames
 * [w * hop, min(w * hop + window, total_rows)) and
 *   counts[w][c], c < num_classes:          frames of the window whose frame_mask has bit c set;
 *   counts[w][c], num_classes <= c < 14:    0;
 *   counts[w][14]:                          frames with any of the bits 0 .. num_classes - 1 set;
 *   counts[w][15]:                          frames of the window inside the timeline (tail windows are short).
 * Bits at or above num_classes are ignored.  A null pointer, total_rows / window / hop / n_windows < 1, num_classes
 * outside 1..SELD_BALANCE_MAX_CLASSES, or a last window that starts behind the end ((n_windows - 1) * hop >=
 * total_rows): -1.  window above 2^31 - 65 or n_windows above 2^31 - 1: -4.  Every refusal comes before any launch. */
#define SELD_BALANCE_COLUMNS 16
#define SELD_BALANCE_MAX_CLASSES 14
int seld_frame_class_mask(const uint16_t* mask, int64_t total_rows, int cells, uint16_t* frame_mask, void* stream);
int seld_window_class_frames(const uint16_t* frame_mask, int64_t total_rows, int64_t window, int64_t hop, int64_t n_windows,
                             int num_classes, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SELD_HIP_H_ */
