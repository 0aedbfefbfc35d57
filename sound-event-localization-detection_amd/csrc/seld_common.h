// Shared host-side plumbing for libseld_hip.so (error reporting, device state).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <string>

#include "logmel_core.h"

namespace seld {

enum : int {
  kOk = 0,
  kErrInvalidArgument = -1,
  kErrHip = -2,
  kErrNotInitialised = -3,
  kErrUnsupported = -4,
};

void set_error(const std::string& msg);
int fail(int code, const std::string& msg);

#define SELD_HIP_TRY(expr)                                                             \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return ::seld::fail(::seld::kErrHip, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

struct DeviceState {
  bool ready = false;
  int device = -1;
  int num_cus = 0;
  // log-mel tables (device memory)
  float* window = nullptr;
  float* twiddle = nullptr;
  int* mel_b0 = nullptr;
  float* mel_wd = nullptr;
  float* mel_wu = nullptr;
  int* mel_pos = nullptr;       // power-row placement (logmel_tables.h, place_power_rows)
  void* gcc_table = nullptr;    // fp16 cosine / sine B fragments of the matrix-core GCC-PHAT (spatial.hip), built by seld_init
  // kernels that need more dynamic LDS than the default limit: hipFuncSetAttribute is per DEVICE (and is not a stream
  // operation: done once so that launches stay graph-capturable); the kernels that have it, see allow_dynamic_lds()
  const void* lds_allowed[32] = {};
  int lds_allowed_n = 0;
  // NIPD tables (device addresses) whose header seld_nipd_q15 has read back and checked, with the span of 16-byte row
  // units their bins cover (nipd.hip): the check is a synchronous read, done once per address
  struct NipdChecked { const void* table; int u_lo, u_cnt; };
  NipdChecked nipd_checked[16] = {};
  int nipd_checked_n = 0, nipd_checked_next = 0;
  LogmelTables tables() const { return LogmelTables{window, twiddle, mel_b0, mel_wd, mel_wu, mel_pos}; }
};

// Lets `kernel` be launched with `bytes` of dynamic LDS: sets the attribute the first time it sees the kernel on this
// device (under the library mutex) and does nothing afterwards.  With the array full it sets it on every call.
int allow_dynamic_lds(DeviceState* st, const void* kernel, int bytes);

// Returns the state of the CURRENT hip device, or nullptr (and sets the error) if seld_init
// has not been called for it.
DeviceState* current_state();

// ---- the host prologue of the entry points that walk spectra or phasors frame by frame (spatial.hip, nipd.hip) ------------
// In this order: the library's state, the pointers, N and F.  Returns kOk with *state set.
inline int check_frame_args(const char* who, std::initializer_list<const void*> pointers, int64_t N, int64_t F,
                            DeviceState** state) {
  const std::string name(who);
  *state = current_state();
  if (!*state) return kErrNotInitialised;
  for (const void* ptr : pointers)
    if (!ptr) return fail(kErrInvalidArgument, name + ": null pointer");
  if (N <= 0 || F <= 0) return fail(kErrInvalidArgument, name + ": N and F must be positive");
  return kOk;
}

// The above, then the channel pairs' own limits: 2..8 channels, a clip's rows of `row_units` each inside 32-bit indices
// (refused as "a clip's <clip_what>") and, where the kernel also indexes frames in 32 bits (`frames32`), N F.
inline int check_pair_args(const char* who, std::initializer_list<const void*> pointers, int64_t N, int64_t C, int64_t F,
                           int64_t row_units, const char* clip_what, bool frames32, DeviceState** state) {
  if (int rc = check_frame_args(who, pointers, N, F, state)) return rc;
  const std::string name(who);
  if (C < 2 || C > 8) return fail(kErrUnsupported, name + ": 2..8 channels");
  if (C * F * row_units >= (1L << 31)) return fail(kErrUnsupported, name + ": a clip's " + clip_what);
  if (frames32 && N * F + 4L * 1024 >= (1L << 31)) return fail(kErrUnsupported, name + ": more than 2^31 frames");
  return kOk;
}

// The pair kernels store four consecutive lags / bands as one vector: unit stride along them, 16-byte aligned rows.
inline bool vector_rows(const void* out, int64_t sN, int64_t sC, int64_t sM, int64_t sT) {
  return sM == 1 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && sN % 4 == 0 && sC % 4 == 0 && sT % 4 == 0;
}

// spatial.hip: the constant fp16 cosine / sine table of the matrix-core GCC-PHAT kernel (96 KB, built by seld_init)
int build_gcc_table(DeviceState* st);

}  // namespace seld
