// Internal helpers shared by the ftmi HIP translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/ftmi.h"

extern char **environ;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define FTMI_CHECK_LAUNCH()                         \
  do {                                              \
    hipError_t e__ = hipGetLastError();             \
    if (e__ != hipSuccess) return (int)e__;         \
  } while (0)

static inline bool ftmi_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

static inline hipStream_t ftmi_hs(ftmi_stream_t s) { return (hipStream_t)s; }

// CUs a persistent grid may count on: the device's, or fewer when a test lowers it
// (ftmi_set_resident_cu_limit; defined in seq.hip)
__attribute__((visibility("hidden"))) int ftmi_resident_cus(void);

// Persistent-launch guard (rnn_bidir, rnn_gemv, highway_stack_spread, wavernn: workgroups
// that wait on each other).  Every workgroup of the grid must be resident at once, so the
// kernel's occupancy at this block size / LDS times the CU count must cover the grid;
// otherwise the caller returns FTMI_E_UNSUPPORTED before launching anything (instead of
// relying on a spin bound to turn the deadlock into a status bit).
static inline int ftmi_resident_ok(const void *kernel, int grid, int block, size_t smem) {
  int per = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, block, smem) != hipSuccess) {
    (void)hipGetLastError();  // a failed query must not surface in the caller's next HIP call
    return FTMI_E_UNSUPPORTED;
  }
  if (per <= 0) return FTMI_E_UNSUPPORTED;
  return (int64_t)per * ftmi_resident_cus() >= grid ? FTMI_OK : FTMI_E_UNSUPPORTED;
}

// Routing switches (gemm.hip Switches, rnn.hip RnnSwitches).  S holds one int64_t per switch
// and then `uint64_t digest` (no padding before it); a table of ftmi_switch<S> has one line
// per switch: a switch added to the table is read, per call, and in the digest without more.
template <class S>
struct ftmi_switch {
  const char *name;
  int64_t S::*field;
  int64_t def;  // -1 by convention: the code's own rule
};
// One pass over the environment (a launch costs one scan, not a getenv per switch); the
// digest is FNV-1a over the bytes before `digest`.
template <class S, size_t N>
static inline S ftmi_read_switches(const ftmi_switch<S> (&table)[N]) {
  S sw = {};
  for (const ftmi_switch<S> &d : table) sw.*d.field = d.def;
  for (char **e = environ; e && *e; ++e) {
    if (strncmp(*e, "FTMI_", 5) != 0) continue;
    const char *eq = strchr(*e, '=');
    if (!eq) continue;
    const size_t n = (size_t)(eq - *e);
    for (const ftmi_switch<S> &d : table)
      if (strlen(d.name) == n && strncmp(*e, d.name, n) == 0) sw.*d.field = atoll(eq + 1);
  }
  sw.digest = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < offsetof(S, digest); ++i)
    sw.digest = (sw.digest ^ ((const unsigned char *)&sw)[i]) * 0x100000001b3ull;
  return sw;
}

__device__ __forceinline__ float ftmi_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// numpy.pad(mode='reflect') index for any pad width (periodic reflection, period 2(L-1));
// shared by the STFT framing (dsp.hip) and the silence trim's frame power (prep.hip)
__device__ __forceinline__ int64_t reflect_index(int64_t j, int64_t L) {
  if (L <= 1) return 0;
  const int64_t per = 2 * (L - 1);
  j %= per;
  if (j < 0) j += per;
  return j >= L ? per - j : j;
}
