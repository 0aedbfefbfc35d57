// Per-channel energy normalisation of the log-mel channels for gfx950.
//
// x is float32 [N][T][C_total][64], time-major; its first C_log channels are log-mel in dB.  Per clip, channel c < C_log and
// bin f (include/seld_hip.h states the arithmetic operation by operation):
//   E[t] = 2^(x[t] log2(10) / 10)                      the mel power back from dB (the -100 dB floor is 1e-10)
//   M[t] = a M[t-1] + s E[t],  a = 1 - s,  M[-1] = E[0]   a first-order smoother along time, restarted in every clip
//   y[t] = (E[t] (eps + M[t])^-alpha + delta)^r - delta^r
// A recurrence along time over a device-resident array: sequential per (clip, channel, bin), so the time axis is cut into
// chunks of SELD_PCEN_CHUNK_FRAMES frames anchored at a clip's frame 0 and the work is two launches on the caller's stream:
//   pcen_carry_kernel   every (clip, chunk that has a successor) walks its 256 frames from state 0 and writes the chunk's
//                       aggregate A_k = sum_i a^(255-i) s E[256 k + i] to the workspace; chunk 0 also writes E[0] there.
//   pcen_apply_kernel   every (clip, chunk) forms its incoming state from the workspace alone -- Horner over the earlier
//                       chunks in ascending order, M <- fmaf(a^256, M, A_j) starting from E[0] -- then walks its frames
//                       with M <- fmaf(a, M, s E) and writes y.
// No spin, no look-back between workgroups, no atomics, no device-scope fence (the second kernel is a second launch on the
// same stream), no LDS, no scratch.  Neither result depends on the grid: a (clip, chunk, lane) is produced by ONE thread
// walking frames and chunks in ascending order.  In place (out == x) the apply kernel reads no frame of another chunk from
// x -- some other workgroup may already have overwritten it -- which is why E[0] travels through the workspace; a lane
// loads a frame before it stores that frame and never touches another lane's bytes.
//
// Layout: the C_log log-mel channels of a frame are C_log * 256 contiguous bytes, so a lane owns one 16-byte unit of a frame
// (4 bins of one channel) and a wavefront 1 KB of it: one wavefront per frame row for C_log = 4, half a wavefront for 2, two
// tiles for 8.  The chunk -- and with it the ragged extent of a clip's last one -- is wave-uniform.  kPcenUnroll frames are
// loaded one step ahead of the dependent fmaf chain (walk_frames), which keeps that many 16-byte loads per lane in flight
// and leaves the order of the arithmetic alone.  Every extent of a chunk is 32-bit; only the frame
// index of the tensor is formed in 64 bits.
#include "seld_common.h"

#include <cmath>

#include "seld_hip.h"

namespace seld {

constexpr int kPcenChunk = SELD_PCEN_CHUNK_FRAMES;
constexpr int kPcenBins = 64;                          // bins per feature channel
constexpr int kPcenUnits = kPcenBins / 4;              // 16-byte units of one channel row
constexpr int kPcenUnroll = 8;
constexpr float kPcenLog2PerDb = 0.33219280948873623f;     // log2(10) / 10
static_assert(kPcenChunk % kPcenUnroll == 0, "a full chunk is a whole number of unrolled steps");

struct PcenParams {
  float s, a, a_chunk;          // a = fl(1 - s); a_chunk = a^256, rounded once from double
  float neg_alpha, delta, r, eps;
  float delta_r;                // delta^r, rounded once from double
};

struct Float4 {
  float v[4];
};

__device__ __forceinline__ Float4 unpack(const uint4 u) {
  return {{__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)}};
}

__device__ __forceinline__ uint4 pack(const Float4& f) {
  return make_uint4(__float_as_uint(f.v[0]), __float_as_uint(f.v[1]), __float_as_uint(f.v[2]), __float_as_uint(f.v[3]));
}

// mel power of a stored dB value: one rounded product, one v_exp_f32
__device__ __forceinline__ float db_power(float x) { return __builtin_amdgcn_exp2f(__fmul_rn(x, kPcenLog2PerDb)); }

// M <- fmaf(a, M, s E) for the four bins of a unit; returns E
__device__ __forceinline__ Float4 smooth(const uint4 u, const PcenParams& p, Float4& m) {
  const Float4 x = unpack(u);
  Float4 e;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    e.v[i] = db_power(x.v[i]);
    m.v[i] = fmaf(p.a, m.v[i], __fmul_rn(p.s, e.v[i]));
  }
  return e;
}

// y = (E (eps + M)^-alpha + delta)^r - delta^r, powers as v_exp_f32 of a rounded multiple of v_log_f32; nothing is contracted
__device__ __forceinline__ uint4 compress(const Float4& e, const Float4& m, const PcenParams& p) {
  Float4 y;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float gain = __builtin_amdgcn_exp2f(__fmul_rn(p.neg_alpha, __builtin_amdgcn_logf(__fadd_rn(p.eps, m.v[i]))));
    const float biased = __fadd_rn(__fmul_rn(e.v[i], gain), p.delta);
    y.v[i] = __fsub_rn(__builtin_amdgcn_exp2f(__fmul_rn(p.r, __builtin_amdgcn_logf(biased))), p.delta_r);
  }
  return pack(y);
}

// body(t, unit of frame t) for t = 0 .. frames - 1 in ascending order; `src` points at this lane's unit of frame 0, frames
// are `stride` units apart.  The loads of step n + 1 (kPcenUnroll frames) are issued before the bodies of step n, and a
// body's own stores (in place: to the addresses its frame was loaded from) come after every load of their step.  `src` is
// deliberately not __restrict__: in place it aliases the destination.
template <typename Body>
__device__ __forceinline__ void walk_frames(const uint4* src, int stride, int frames, Body&& body) {
  uint4 cur[kPcenUnroll];
  int t = 0;
  if (frames >= kPcenUnroll) {
#pragma unroll
    for (int u = 0; u < kPcenUnroll; ++u) cur[u] = src[static_cast<long>(u) * stride];
  }
  for (; t + kPcenUnroll <= frames; t += kPcenUnroll) {
    uint4 nxt[kPcenUnroll];
    const bool more = t + 2 * kPcenUnroll <= frames;
    if (more) {
#pragma unroll
      for (int u = 0; u < kPcenUnroll; ++u) nxt[u] = src[static_cast<long>(t + kPcenUnroll + u) * stride];
    }
#pragma unroll
    for (int u = 0; u < kPcenUnroll; ++u) body(t + u, cur[u]);
    if (more) {
#pragma unroll
      for (int u = 0; u < kPcenUnroll; ++u) cur[u] = nxt[u];
    }
  }
  for (; t < frames; ++t) body(t, src[static_cast<long>(t) * stride]);
}

// (clip, chunk, tile) of a work item; false when this lane's unit lies past the log-mel channels
struct PcenItem {
  int clip, chunk, unit;
};

__device__ __forceinline__ bool pcen_item(int item, int chunks, int tiles, int log_units, PcenItem* it) {
  const int per_clip = chunks * tiles;
  it->clip = item / per_clip;
  const int rest = item - it->clip * per_clip;
  it->chunk = rest / tiles;
  it->unit = (rest - it->chunk * tiles) * 64 + static_cast<int>(threadIdx.x);
  return it->unit < log_units;
}

// workspace: float [N][n_chunks][log_units * 4]; row 0 of a clip is E[0], row 1 + k the aggregate of chunk k < n_chunks - 1.
// Items: N * max(n_chunks - 1, 1) * tiles -- the chunks that have a successor (all of them full), or chunk 0 alone for E[0].
__global__ void __launch_bounds__(64)
pcen_carry_kernel(const uint4* __restrict__ x, int items, int T, int n_chunks, int walked, int row_units, int log_units,
                  int tiles, PcenParams p, uint4* __restrict__ ws) {
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    PcenItem it;
    if (!pcen_item(item, walked, tiles, log_units, &it)) continue;
    const uint4* __restrict__ src = x + (static_cast<long>(it.clip) * T + it.chunk * kPcenChunk) * row_units + it.unit;
    uint4* __restrict__ rows = ws + static_cast<long>(it.clip) * n_chunks * log_units + it.unit;
    if (it.chunk == 0) {
      const Float4 x0 = unpack(src[0]);
      rows[0] = pack(Float4{{db_power(x0.v[0]), db_power(x0.v[1]), db_power(x0.v[2]), db_power(x0.v[3])}});
    }
    if (it.chunk >= n_chunks - 1) continue;            // a clip's last chunk has no successor: nobody reads its aggregate
    Float4 m = {{0.0f, 0.0f, 0.0f, 0.0f}};
    walk_frames(src, row_units, kPcenChunk, [&](int, const uint4 u) { smooth(u, p, m); });
    rows[static_cast<long>(1 + it.chunk) * log_units] = pack(m);
  }
}

// Items: N * n_chunks * tiles.  x and out may be the same pointer.
__global__ void __launch_bounds__(64)
pcen_apply_kernel(const uint4* x, uint4* out, int items, int T, int n_chunks, int last_frames, int row_units, int log_units,
                  int tiles, PcenParams p, const uint4* __restrict__ ws) {
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    PcenItem it;
    if (!pcen_item(item, n_chunks, tiles, log_units, &it)) continue;
    const uint4* __restrict__ rows = ws + static_cast<long>(it.clip) * n_chunks * log_units + it.unit;
    Float4 m = unpack(rows[0]);                        // M[-1] = E[0]
    int j = 0;
    for (; j + kPcenUnroll <= it.chunk; j += kPcenUnroll) {
      uint4 agg[kPcenUnroll];
#pragma unroll
      for (int u = 0; u < kPcenUnroll; ++u) agg[u] = rows[static_cast<long>(1 + j + u) * log_units];
#pragma unroll
      for (int u = 0; u < kPcenUnroll; ++u) {
        const Float4 a = unpack(agg[u]);
#pragma unroll
        for (int i = 0; i < 4; ++i) m.v[i] = fmaf(p.a_chunk, m.v[i], a.v[i]);
      }
    }
    for (; j < it.chunk; ++j) {
      const Float4 a = unpack(rows[static_cast<long>(1 + j) * log_units]);
#pragma unroll
      for (int i = 0; i < 4; ++i) m.v[i] = fmaf(p.a_chunk, m.v[i], a.v[i]);
    }
    const int frames = it.chunk == n_chunks - 1 ? last_frames : kPcenChunk;
    const long first = (static_cast<long>(it.clip) * T + it.chunk * kPcenChunk) * row_units + it.unit;
    uint4* dst = out + first;
    walk_frames(x + first, row_units, frames, [&](int t, const uint4 u) {
      const Float4 e = smooth(u, p, m);
      dst[static_cast<long>(t) * row_units] = compress(e, m, p);
    });
  }
}

// chunks of a clip, or -1 when the extents are refused or a kernel's 32-bit item count would overflow
static int64_t pcen_chunks(int64_t N, int64_t T, int C_total, int C_log) {
  if (N < 1 || T < 1 || C_log < 1 || C_log > C_total || C_total > (1 << 20)) return -1;    // C_total * 16 row units: an int
  if (T >= (int64_t{1} << 31) - kPcenChunk) return -1;                                      // a clip's frames: an int
  const int64_t chunks = (T + kPcenChunk - 1) / kPcenChunk;
  const int64_t tiles = (static_cast<int64_t>(C_log) * kPcenUnits + 63) / 64;
  if (N > ((int64_t{1} << 31) - 1) / (chunks * tiles)) return -1;
  return chunks;
}

}  // namespace seld

extern "C" {

int64_t seld_pcen_workspace(int64_t N, int64_t T, int C_total, int C_log) {
  const int64_t chunks = seld::pcen_chunks(N, T, C_total, C_log);
  if (chunks < 0) return 0;
  return N * chunks * C_log * seld::kPcenBins * static_cast<int64_t>(sizeof(float));
}

int seld_pcen(const float* x, float* out, int64_t N, int64_t T, int C_total, int C_log, float s, float alpha, float delta,
              float r, float eps, void* workspace, int64_t workspace_bytes, void* stream_) {
  using namespace seld;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (!x || !out || !workspace) return fail(kErrInvalidArgument, "seld_pcen: null pointer");
  if (N < 1 || T < 1) return fail(kErrInvalidArgument, "seld_pcen: N and T must be at least 1");
  if (C_log < 1 || C_log > C_total)
    return fail(kErrInvalidArgument, "seld_pcen: C_log must be in 1..C_total (the leading log-mel channels)");
  for (const float v : {s, alpha, delta, r, eps})
    if (!std::isfinite(v)) return fail(kErrInvalidArgument, "seld_pcen: s, alpha, delta, r and eps must be finite");
  if (!(s > 0.0f && s <= 1.0f)) return fail(kErrInvalidArgument, "seld_pcen: s must be in (0, 1]");
  if (!(alpha >= 0.0f && alpha <= 1.0f)) return fail(kErrInvalidArgument, "seld_pcen: alpha must be in [0, 1]");
  if (!(r > 0.0f && r <= 1.0f)) return fail(kErrInvalidArgument, "seld_pcen: r must be in (0, 1]");
  if (!(delta > 0.0f && eps > 0.0f)) return fail(kErrInvalidArgument, "seld_pcen: delta and eps must be positive");
  const int64_t chunks = pcen_chunks(N, T, C_total, C_log);
  if (chunks < 0) return fail(kErrUnsupported, "seld_pcen: clip too long, too many clips or too many channels");
  if (workspace_bytes < seld_pcen_workspace(N, T, C_total, C_log))
    return fail(kErrInvalidArgument, "seld_pcen: workspace smaller than seld_pcen_workspace reports");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace)) & 15)
    return fail(kErrUnsupported, "seld_pcen: x, out and workspace must be 16-byte aligned");
  const int64_t floats = N * T * C_total * kPcenBins;
  if (out != x && out < x + floats && x < out + floats)
    return fail(kErrInvalidArgument, "seld_pcen: out must be x itself or not overlap it");
  hipStream_t stream = static_cast<hipStream_t>(stream_);

  PcenParams p;
  p.s = s;
  p.a = 1.0f - s;
  p.a_chunk = static_cast<float>(std::pow(static_cast<double>(p.a), static_cast<double>(kPcenChunk)));
  p.neg_alpha = -alpha;
  p.delta = delta;
  p.r = r;
  p.eps = eps;
  p.delta_r = static_cast<float>(std::pow(static_cast<double>(delta), static_cast<double>(r)));

  const int n_chunks = static_cast<int>(chunks);
  const int last_frames = static_cast<int>(T - (chunks - 1) * kPcenChunk);
  const int row_units = C_total * kPcenUnits, log_units = C_log * kPcenUnits;
  const int tiles = (log_units + 63) / 64;
  const int walked = n_chunks > 1 ? n_chunks - 1 : 1;
  const int64_t cap = static_cast<int64_t>(st->num_cus) * 32;       // one-wave blocks: up to 8 per SIMD
  const int64_t carry_items = N * walked * tiles, apply_items = N * chunks * tiles;
  hipLaunchKernelGGL(pcen_carry_kernel, dim3(static_cast<unsigned>(carry_items < cap ? carry_items : cap)), dim3(64), 0,
                     stream, reinterpret_cast<const uint4*>(x), static_cast<int>(carry_items), static_cast<int>(T), n_chunks,
                     walked, row_units, log_units, tiles, p, static_cast<uint4*>(workspace));
  SELD_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(pcen_apply_kernel, dim3(static_cast<unsigned>(apply_items < cap ? apply_items : cap)), dim3(64), 0,
                     stream, reinterpret_cast<const uint4*>(x), reinterpret_cast<uint4*>(out), static_cast<int>(apply_items),
                     static_cast<int>(T), n_chunks, last_frames, row_units, log_units, tiles, p,
                     static_cast<const uint4*>(workspace));
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
