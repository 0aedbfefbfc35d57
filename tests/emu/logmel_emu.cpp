// TEST TOOL (not shipped, not linked into libseld_hip.so): runs the log-mel kernel's per-lane
// phase functions (csrc/logmel_core.h) on the CPU, 64 "lanes" in lock step with a plain array
// standing in for the wavefront's LDS tile.  It lets the CPU test-suite check the kernel's
// index math (32x30 factorisation, packed-frame un-mixing, sparse mel ownership, reflection at
// the clip edges) against the oracle without a GPU.  The product never calls this.
//
//   g++ -O2 -shared -fPIC -I <csrc> tests/emu/logmel_emu.cpp -o tests/emu/libseld_emu.so
#include <stdint.h>
#include <string.h>

#include <vector>

#include "logmel_core.h"
#include "logmel_tables.h"

using namespace seld;

namespace {

struct HostTables {
  std::vector<float> window, twiddle, fb, wd, wu;
  std::vector<int> b0, pos;
  LogmelTables view() const {
    return LogmelTables{window.data(), twiddle.data(), b0.data(), wd.data(), wu.data(), pos.data()};
  }
};

constexpr int kGuard = 64;
const float kGuardValue = -12345.0f;

// The verdict of the all-zero rule for the half-wavefront of ``lane`` (csrc/logmel.hip pair_live: two ballots): a frame is
// live if any lane of the half holds a non-zero sample of it.  ``rule`` 0 = the core as it was before the rule (every
// frame live), which the CPU suite compares against.
void pair_live(const std::vector<unsigned>& bits, int lane, int rule, bool& live_a, bool& live_b) {
  unsigned any = 0;
  for (int l = 0; l < 32; ++l) any |= bits[(lane & 32) + l];
  live_a = !rule || (any & kLiveA) != 0;
  live_b = !rule || (any & kLiveB) != 0;
}

// kSpec as in csrc/logmel.hip: 0 = log-mel only, 1 = the un-packed spectra as well ([rows][F][481] complex64), 2 = the Q15
// phasor words ([rows][F][kPhasorPitch]).  The wavefront's tile sits between guard cells: an LDS index that leaves it -> -9.
template <typename T, int kSpec>
int run(const T* pcm, int64_t N, int64_t C, int64_t L, float* out, long sN, long sC, long sM, long sT, const float* fb_opt,
        void* spec, int rule) {
  if (L <= kNfft / 2) return -1;
  HostTables t;
  hann_window(t.window);
  stage_twiddles(t.twiddle);
  if (fb_opt)
    t.fb.assign(fb_opt, fb_opt + static_cast<size_t>(kBins) * kMels);
  else
    default_mel_filterbank(t.fb);
  if (build_sparse_mel(t.fb, t.b0, t.wd, t.wu)) return -4;
  if (place_power_rows(t.fb, t.b0, t.pos)) return -5;
  const LogmelTables tab = t.view();

  const IterGeometry g = iter_geometry(L);
  const long F = g.F;
  std::vector<float> block(kGuard + kLdsFloatsPerWave + kGuard, 0.0f);
  for (int i = 0; i < kGuard; ++i) block[i] = block[block.size() - 1 - i] = kGuardValue;
  float* lds = block.data() + kGuard;
  std::vector<float> tab_lds(kTabFloats);
  for (int e = 0; e < kTabFloats; ++e) tab_lds[e] = table_value(tab, e);
  std::vector<cf> z(64 * kN2), m(64 * 16);
  std::vector<float> smp(64 * 48);
  std::vector<unsigned> bits(64);
  std::vector<LaneAcc> acc(64);

  for (long row = 0; row < N * C; ++row) {
    const T* rowp = pcm + row * L;
    const long n = row / C, c = row % C;
    for (long itr = 0; itr < g.iters_per_row; ++itr) {
      const long tf = itr * kFramesPerIter;
      const bool interior = g.is_interior(itr);
      for (int lane = 0; lane < 64; ++lane) {
        const long fa = tf + 2 * (lane >> 5);
        float(&s)[48] = *reinterpret_cast<float(*)[48]>(&smp[lane * 48]);
        if (interior) load_samples<T, true>(lane, rowp, L, fa, s);
        else load_samples<T, false>(lane, rowp, L, fa, s);
        bits[lane] = lane_live_bits(s);
      }
      for (int lane = 0; lane < 64; ++lane) {
        LaneConsts consts;
        load_lane_consts(lane, tab_lds.data(), consts);
        phase_a(lane, *reinterpret_cast<float(*)[48]>(&smp[lane * 48]), consts, lds);
      }
      for (int lane = 0; lane < 64; ++lane)
        phase_b(lane, lds, *reinterpret_cast<cf(*)[kN2]>(&z[lane * kN2]));
      for (int lane = 0; lane < 64; ++lane)
        phase_b_store(lane, lds, *reinterpret_cast<cf(*)[kN2]>(&z[lane * kN2]));
      for (int lane = 0; lane < 64; ++lane)
        phase_c_load(lane, lds, *reinterpret_cast<cf(*)[16]>(&m[lane * 16]));
      for (int lane = 0; lane < 64; ++lane) {
        const int h = lane >> 5;
        const long fa = tf + 2 * h;
        bool live_a, live_b;
        pair_live(bits, lane, rule, live_a, live_b);
        const cf(&zl)[kN2] = *reinterpret_cast<cf(*)[kN2]>(&z[lane * kN2]);
        const cf(&ml)[16] = *reinterpret_cast<cf(*)[16]>(&m[lane * 16]);
        float* pp[16];
        power_row_pointers(lane, lds, t.pos.data(), pp);
        if (kSpec == 1) {                                    // as edge_iteration: frames past the end are not stored
          float* base = static_cast<float*>(spec) + (row * F + fa) * (2 * kBins);
          phase_c_spectrum(lane, zl, ml, fa < F ? base : nullptr, fa + 1 < F ? base + 2 * kBins : nullptr);
          phase_c_zero_spectrum(lane, fa < F ? base : nullptr, fa + 1 < F ? base + 2 * kBins : nullptr, live_a, live_b);
        }
        if (kSpec == 2) {
          unsigned* base = static_cast<unsigned*>(spec) + (row * F + tf) * kPhasorPitch;
          const unsigned off_a = static_cast<unsigned>(2 * h * kPhasorPitch + (lane & 31));
          phase_c_store_phasors(lane, pp, zl, ml, base, off_a, fa < F, fa + 1 < F);
          phase_c_zero_phasors(lane, base, off_a, fa < F, fa + 1 < F, live_a, live_b);
        } else {
          phase_c_store(lane, pp, zl, ml);
        }
        phase_c_zero_rows(lane, pp, live_a, live_b);
      }
      for (int lane = 0; lane < 64; ++lane)
        phase_d_accumulate(lane, lds, tab_lds.data(), t.pos[lane], acc[lane]);
      for (int lane = 0; lane < 64; ++lane) {
        float db[kFramesPerIter];
        float below[kFramesPerIter];
        for (int s = 0; s < kFramesPerIter; ++s) below[s] = lane > 0 ? acc[lane - 1].ab[s].y : 0.0f;
        phase_d_finish(acc[lane], below, db);
        float* outp = out + n * sN + c * sC + lane * sM;
        for (int s = 0; s < kFramesPerIter; ++s)
          if (tf + s < F) outp[(tf + s) * sT] = db[s];
      }
    }
  }
  for (int i = 0; i < kGuard; ++i)
    if (block[i] != kGuardValue || block[block.size() - 1 - i] != kGuardValue) return -9;     // an LDS index left the tile
  return 0;
}

template <typename T>
int run_layout(const T* pcm, int64_t N, int64_t C, int64_t L, float* out, int layout, const float* fb_opt) {
  const long F = 1 + L / kHop;
  if (layout == 0) return run<T, 0>(pcm, N, C, L, out, C * kMels * F, kMels * F, F, 1, fb_opt, nullptr, 1);
  return run<T, 0>(pcm, N, C, L, out, F * C * kMels, kMels, 1, C * kMels, fb_opt, nullptr, 1);
}

// The fused FOA pass (csrc/logmel.hip logmel_iv_kernel): four "wavefronts" = channels W, X, Y, Z of one clip in lock step,
// their tiles contiguous as in the kernel's LDS, W's spectrum buffer behind them.  Every LDS index the per-lane functions
// form is kept honest by guard cells either side of the block (writes) and by the comparison with the oracle (reads).
template <typename T>
int run_iv(const T* pcm, int64_t N, int64_t L, float* out, const float* fb_opt, int rule) {
  if (L <= kNfft / 2) return -1;
  HostTables t;
  hann_window(t.window);
  stage_twiddles(t.twiddle);
  if (fb_opt)
    t.fb.assign(fb_opt, fb_opt + static_cast<size_t>(kBins) * kMels);
  else
    default_mel_filterbank(t.fb);
  if (build_sparse_mel(t.fb, t.b0, t.wd, t.wu)) return -4;
  if (place_power_rows(t.fb, t.b0, t.pos)) return -5;
  const LogmelTables tab = t.view();
  const IterGeometry g = iter_geometry(L);
  const long F = g.F;
  const long total_ch = 2 * kIvChannels - 1;
  const long sM = 1, sC = kMels, sT = total_ch * kMels, sN = F * total_ch * kMels;
  std::vector<float> block(kGuard + kIvChannels * kLdsFloatsPerWave + kIvSpecFloats + kGuard, 0.0f);
  for (int i = 0; i < kGuard; ++i) block[i] = block[block.size() - 1 - i] = kGuardValue;
  float* tiles = block.data() + kGuard;
  float* wspec = tiles + kIvChannels * kLdsFloatsPerWave;
  std::vector<float> tab_lds(kTabFloats);
  for (int e = 0; e < kTabFloats; ++e) tab_lds[e] = table_value(tab, e);
  std::vector<cf> z(kIvChannels * 64 * kN2), m(kIvChannels * 64 * 16), xa(kIvChannels * 64 * 16), xb(kIvChannels * 64 * 16);
  std::vector<float> smp(64 * 48), ia(kIvChannels * 64 * 16), ib(kIvChannels * 64 * 16);
  std::vector<LaneAcc> acc(64);
  std::vector<unsigned> bits(64);
#define AT(vec, w, lane, n) (*reinterpret_cast<decltype(vec)::value_type(*)[n]>(&vec[((w) * 64 + (lane)) * (n)]))
  for (long clip = 0; clip < N; ++clip) {
    for (long itr = 0; itr < g.iters_per_row; ++itr) {
      const long tf = itr * kFramesPerIter;
      const bool interior = g.is_interior(itr);
      for (int w = 0; w < kIvChannels; ++w) {
        float* lds = tiles + w * kLdsFloatsPerWave;
        const T* rowp = pcm + (clip * kIvChannels + w) * L;
        for (int lane = 0; lane < 64; ++lane) {
          float(&s)[48] = *reinterpret_cast<float(*)[48]>(&smp[lane * 48]);
          const long fa = tf + 2 * (lane >> 5);
          if (interior) load_samples<T, true>(lane, rowp, L, fa, s);
          else load_samples<T, false>(lane, rowp, L, fa, s);
          bits[lane] = lane_live_bits(s);
        }
        for (int lane = 0; lane < 64; ++lane) {
          LaneConsts consts;
          load_lane_consts(lane, tab_lds.data(), consts);
          phase_a(lane, *reinterpret_cast<float(*)[48]>(&smp[lane * 48]), consts, lds);
        }
        for (int lane = 0; lane < 64; ++lane) phase_b(lane, lds, AT(z, w, lane, kN2));
        for (int lane = 0; lane < 64; ++lane) phase_b_store(lane, lds, AT(z, w, lane, kN2));
        for (int lane = 0; lane < 64; ++lane) phase_c_load(lane, lds, AT(m, w, lane, 16));
        for (int lane = 0; lane < 64; ++lane) {
          float* pp[16];
          power_row_pointers(lane, lds, t.pos.data(), pp);
          bool live_a, live_b;
          pair_live(bits, lane, rule, live_a, live_b);
          phase_c_unpack(lane, pp, AT(z, w, lane, kN2), AT(m, w, lane, 16), AT(xa, w, lane, 16), AT(xb, w, lane, 16));
          phase_c_zero_unpacked(lane, pp, AT(xa, w, lane, 16), AT(xb, w, lane, 16), live_a, live_b);
        }
        if (w == 0)
          for (int lane = 0; lane < 64; ++lane) iv_publish(lane, wspec, AT(xa, 0, lane, 16), AT(xb, 0, lane, 16));
      }
      // ---- workgroup barrier 1
      for (int w = 1; w < kIvChannels; ++w) {
        float* lds = tiles + w * kLdsFloatsPerWave;
        for (int lane = 0; lane < 64; ++lane) {
          float* pp[16];
          power_row_pointers(lane, lds, t.pos.data(), pp);
          iv_compute(lane, w, wspec, pp, AT(xa, w, lane, 16), AT(xb, w, lane, 16), 1e-8f, AT(ia, w, lane, 16), AT(ib, w, lane, 16));
        }
      }
      for (int w = 0; w < kIvChannels; ++w) {
        float* lds = tiles + w * kLdsFloatsPerWave;
        for (int lane = 0; lane < 64; ++lane) phase_d_accumulate(lane, lds, tab_lds.data(), t.pos[lane], acc[lane]);
        for (int lane = 0; lane < 64; ++lane) {
          float db[kFramesPerIter], below[kFramesPerIter];
          for (int s = 0; s < kFramesPerIter; ++s) below[s] = lane > 0 ? acc[lane - 1].ab[s].y : 0.0f;
          phase_d_finish(acc[lane], below, db);
          float* outp = out + clip * sN + w * sC + lane * sM;
          for (int s = 0; s < kFramesPerIter; ++s)
            if (tf + s < F) outp[(tf + s) * sT] = db[s];
        }
      }
      // ---- workgroup barrier 2
      for (int w = 1; w < kIvChannels; ++w) {
        float* lds = tiles + w * kLdsFloatsPerWave;
        for (int lane = 0; lane < 64; ++lane) {
          float* pp[16];
          power_row_pointers(lane, lds, t.pos.data(), pp);
          iv_store_rows(lane, pp, AT(ia, w, lane, 16), AT(ib, w, lane, 16));
        }
        for (int lane = 0; lane < 64; ++lane) phase_d_accumulate(lane, lds, tab_lds.data(), t.pos[lane], acc[lane]);
        for (int lane = 0; lane < 64; ++lane) {
          float* outp = out + clip * sN + (kIvChannels - 1 + w) * sC + lane * sM;
          for (int s = 0; s < kFramesPerIter; ++s)
            if (tf + s < F) outp[(tf + s) * sT] = acc[lane].ab[s].x + (lane > 0 ? acc[lane - 1].ab[s].y : 0.0f);
        }
      }
    }
  }
#undef AT
  for (int i = 0; i < kGuard; ++i)
    if (block[i] != kGuardValue || block[block.size() - 1 - i] != kGuardValue) return -9;     // an LDS index left the block
  return 0;
}

}  // namespace

extern "C" {
int emu_logmel_f32(const float* pcm, int64_t N, int64_t C, int64_t L, float* out, int layout, const float* fb) {
  return run_layout<float>(pcm, N, C, L, out, layout, fb);
}
int emu_logmel_i16(const int16_t* pcm, int64_t N, int64_t C, int64_t L, float* out, int layout, const float* fb) {
  return run_layout<int16_t>(pcm, N, C, L, out, layout, fb);
}
// The phasor and spectrum exports with the arguments of seld_logmel_phasors_* / seld_logmel_spectrum_* (include/seld_hip.h),
// the filterbank and ``rule`` (1 = the all-zero rule of logmel_core.h, 0 = the core without it) in the stream's place.
int emu_logmel_phasors_f32(const float* pcm, int64_t N, int64_t C, int64_t L, float* out, int64_t sN, int64_t sC, int64_t sM,
                           int64_t sT, uint32_t* phasors_q15, const float* fb, int rule) {
  return run<float, 2>(pcm, N, C, L, out, sN, sC, sM, sT, fb, phasors_q15, rule);
}
int emu_logmel_phasors_i16(const int16_t* pcm, int64_t N, int64_t C, int64_t L, float* out, int64_t sN, int64_t sC, int64_t sM,
                           int64_t sT, uint32_t* phasors_q15, const float* fb, int rule) {
  return run<int16_t, 2>(pcm, N, C, L, out, sN, sC, sM, sT, fb, phasors_q15, rule);
}
int emu_logmel_spectrum_f32(const float* pcm, int64_t N, int64_t C, int64_t L, float* out, int64_t sN, int64_t sC, int64_t sM,
                            int64_t sT, float* spec_complex, const float* fb, int rule) {
  return run<float, 1>(pcm, N, C, L, out, sN, sC, sM, sT, fb, spec_complex, rule);
}
int emu_logmel_spectrum_i16(const int16_t* pcm, int64_t N, int64_t C, int64_t L, float* out, int64_t sN, int64_t sC, int64_t sM,
                            int64_t sT, float* spec_complex, const float* fb, int rule) {
  return run<int16_t, 1>(pcm, N, C, L, out, sN, sC, sM, sT, fb, spec_complex, rule);
}
int64_t emu_phasor_pitch(void) { return kPhasorPitch; }
// pcm [N][4][L] -> out [N][F][7][64]: log-mel of W, X, Y, Z and the three intensity-vector channels (fused FOA pass)
int emu_logmel_iv_f32(const float* pcm, int64_t N, int64_t L, float* out, const float* fb) {
  return run_iv<float>(pcm, N, L, out, fb, 1);
}
int emu_logmel_iv_i16(const int16_t* pcm, int64_t N, int64_t L, float* out, const float* fb) {
  return run_iv<int16_t>(pcm, N, L, out, fb, 1);
}
int emu_logmel_iv_rule_f32(const float* pcm, int64_t N, int64_t L, float* out, const float* fb, int rule) {
  return run_iv<float>(pcm, N, L, out, fb, rule);
}
}
