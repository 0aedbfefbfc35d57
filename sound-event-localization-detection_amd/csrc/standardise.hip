// Per-bin feature standardisation for gfx950: the moments of the training timeline.
//
// SELDDataset.spec_tm is float32 [total_rows][channels][64], time-major.  Standardising every (channel, bin) column needs
// sum x and sum x^2 over the frames -- a reduction over a device-resident array of up to several GB that runs once per
// training run.  The APPLICATION of the statistics is no kernel of its own: it is the kAffine instantiation of the three
// window gathers (labels.hip, augment.hip, rotate.hip; augment_core.h, standardised).
//
// The summation order is part of the interface (include/seld_hip.h), because every rank of a data-parallel run computes the
// statistics from its own copy of the timeline and the ranks must agree bit for bit without a collective:
//   slab partial[s][k][col] = fp64 sum over the frames of slab s (SELD_MOMENT_SLAB_FRAMES each, the last ragged), ascending,
//                             from 0.0, of x (k = 0) or of the fp64 product x * x (k = 1), x widened to fp64 first;
//   moments[k][col]         = fp64 sum over the slabs, ascending, from 0.0.
// Neither depends on the grid: a (slab, column) partial is produced by ONE thread walking the slab's frames in order, and a
// result by one thread walking the slabs in order.  No atomics, no device-scope fence (the second kernel is a second
// launch on the same stream), no LDS, no scratch.
//
// moment_slab_kernel: one wavefront per (slab, tile of 64 16-byte chunks of a row), so the slab -- and with it the ragged
// extent of the last one -- is wave-uniform and a wavefront's loads of a frame are 1024 contiguous bytes.  A lane owns four
// columns (one uint4 of every frame) and 8 fp64 accumulators; kMomentUnroll frames are loaded before their sums, which keeps
// that many 16-byte loads per lane in flight and leaves the order of the additions alone.  The timeline is read once.
#include "seld_common.h"

#include "seld_hip.h"

namespace seld {

constexpr int kSlabFrames = SELD_MOMENT_SLAB_FRAMES;
constexpr int kMomentBins = 64;                        // bins per feature channel
constexpr int kMomentChunks = kMomentBins / 4;         // 16-byte chunks of one channel row
constexpr int kMomentUnroll = 8;
static_assert(kSlabFrames % kMomentUnroll == 0, "a full slab is a whole number of unrolled steps");

// acc += x and acc2 += x * x for the four floats of a chunk, each sum rounded on its own
__device__ __forceinline__ void add_chunk(const uint4 v, double (&s1)[4], double (&s2)[4]) {
  const double x[4] = {static_cast<double>(__uint_as_float(v.x)), static_cast<double>(__uint_as_float(v.y)),
                       static_cast<double>(__uint_as_float(v.z)), static_cast<double>(__uint_as_float(v.w))};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    s1[e] = __dadd_rn(s1[e], x[e]);
    s2[e] = __dadd_rn(s2[e], __dmul_rn(x[e], x[e]));
  }
}

// partial: double [n_slabs][2][row_chunks * 4].  Every extent here is 32-bit (host: n_slabs * tiles < 2^31); only the
// frame index of the timeline is formed in 64 bits.
__global__ void __launch_bounds__(64)
moment_slab_kernel(const uint4* __restrict__ src, int n_slabs, int last_frames, int row_chunks, int tiles,
                   double* __restrict__ partial) {
  const int items = n_slabs * tiles;
  const int columns = row_chunks * 4;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int slab = item / tiles;
    const int chunk = (item - slab * tiles) * 64 + static_cast<int>(threadIdx.x);
    if (chunk >= row_chunks) continue;
    const int frames = slab == n_slabs - 1 ? last_frames : kSlabFrames;
    const uint4* __restrict__ p = src + (static_cast<long>(slab) * kSlabFrames) * row_chunks + chunk;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    int t = 0;
    for (; t + kMomentUnroll <= frames; t += kMomentUnroll) {
      uint4 v[kMomentUnroll];
#pragma unroll
      for (int u = 0; u < kMomentUnroll; ++u) v[u] = p[static_cast<long>(t + u) * row_chunks];
#pragma unroll
      for (int u = 0; u < kMomentUnroll; ++u) add_chunk(v[u], s1, s2);
    }
    for (; t < frames; ++t) add_chunk(p[static_cast<long>(t) * row_chunks], s1, s2);
    double* __restrict__ out = partial + static_cast<long>(slab) * 2 * columns + chunk * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      out[e] = s1[e];
      out[columns + e] = s2[e];
    }
  }
}

// moments[j] = sum over the slabs, ascending, of partial[s][j], j over the 2 * columns results
__global__ void __launch_bounds__(256)
moment_fold_kernel(const double* __restrict__ partial, int n_slabs, int results, double* __restrict__ moments) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < results; j += gridDim.x * blockDim.x) {
    double acc = 0.0;
    for (int s = 0; s < n_slabs; ++s) acc = __dadd_rn(acc, partial[static_cast<long>(s) * results + j]);
    moments[j] = acc;
  }
}

// slabs of a timeline, or -1 when the extents are refused or the 32-bit item count of the slab kernel would overflow
static int64_t moment_slabs(int64_t total_rows, int channels) {
  if (total_rows <= 0 || channels <= 0 || channels > (1 << 20)) return -1;   // 2 * channels * 64 results: an int
  const int64_t slabs = (total_rows + kSlabFrames - 1) / kSlabFrames;
  const int64_t tiles = (static_cast<int64_t>(channels) * kMomentChunks + 63) / 64;
  if (slabs > ((int64_t{1} << 31) - 1) / tiles) return -1;
  return slabs;
}

}  // namespace seld

extern "C" {

int64_t seld_feature_moments_workspace(int64_t total_rows, int channels) {
  const int64_t slabs = seld::moment_slabs(total_rows, channels);
  if (slabs < 0) return 0;
  return slabs * 2 * channels * seld::kMomentBins * static_cast<int64_t>(sizeof(double));
}

int seld_feature_moments(const float* src, int64_t total_rows, int channels, double* moments, void* workspace,
                         int64_t workspace_bytes, void* stream_) {
  using namespace seld;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (total_rows <= 0)
    return fail(kErrInvalidArgument, "seld_feature_moments: total_rows must be positive (no statistics of an empty timeline)");
  if (channels <= 0) return fail(kErrInvalidArgument, "seld_feature_moments: channels must be positive");
  if (!src || !moments || !workspace) return fail(kErrInvalidArgument, "seld_feature_moments: null pointer");
  const int64_t slabs = moment_slabs(total_rows, channels);
  if (slabs < 0) return fail(kErrUnsupported, "seld_feature_moments: timeline too long or too many channels");
  if (workspace_bytes < seld_feature_moments_workspace(total_rows, channels))
    return fail(kErrInvalidArgument, "seld_feature_moments: workspace smaller than seld_feature_moments_workspace reports");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int row_chunks = channels * kMomentChunks;
  const int tiles = (row_chunks + 63) / 64;
  const int n_slabs = static_cast<int>(slabs);
  const int last_frames = static_cast<int>(total_rows - (slabs - 1) * kSlabFrames);
  const int64_t items = slabs * tiles;
  const int64_t cap = static_cast<int64_t>(st->num_cus) * 32;       // one-wave blocks: up to 8 per SIMD
  const unsigned blocks = static_cast<unsigned>(items < cap ? items : cap);
  hipLaunchKernelGGL(moment_slab_kernel, dim3(blocks), dim3(64), 0, stream, reinterpret_cast<const uint4*>(src), n_slabs,
                     last_frames, row_chunks, tiles, static_cast<double*>(workspace));
  SELD_HIP_TRY(hipGetLastError());
  const int results = 2 * row_chunks * 4;
  hipLaunchKernelGGL(moment_fold_kernel, dim3(static_cast<unsigned>((results + 255) / 256)), dim3(256), 0, stream,
                     static_cast<const double*>(workspace), n_slabs, results, moments);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
