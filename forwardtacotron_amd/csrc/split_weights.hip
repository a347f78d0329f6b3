// The weight and activation-row splitters of the bf16x6 and f16x3 paths.
#include "gemm.h"

using namespace ftmi_gemm;

namespace {

// w [N][K] fp32 -> [3][N][Kpad] bf16 pieces (w = p0 + p1 + p2 exactly), zero K padding
__global__ void split_weights_kernel(const float *__restrict__ w, int64_t N, int64_t K,
                                     int64_t Kpad, __bf16 *__restrict__ out) {
  const int64_t total = N * Kpad;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / Kpad, k = i - n * Kpad;
    const float v = k < K ? w[n * K + k] : 0.f;
    const __bf16 h1 = (__bf16)v;
    const float r1 = v - (float)h1;
    const __bf16 h2 = (__bf16)r1;
    const __bf16 h3 = (__bf16)(r1 - (float)h2);
    out[i] = h1;
    out[total + i] = h2;
    out[2 * total + i] = h3;
  }
}

// w [N][K] fp32 -> f16 planes [3][N][Kpad] (B0 = 2^11 w_h, B1 = w_t, B2 = w_h of the
// column-scaled row w s_n) followed by colscale[N] = 2^-11 / s_n.  One workgroup per row:
// s_n = 2^-e normalises the row, 8 <= max|w[n]| s_n < 16 (e >= -100; an all-zero row: e = 0):
// 2^11 w_h stays inside the f16 range, and a row of small weights is scaled UP, so its heads
// and tails are normal f16 numbers (with e >= 0 only, a row below ~2^-17 lost its tails to the
// f16 subnormal spacing: 7e-5 relative on a 2^-20-sized row).
// frag: planes in the fragment-major order [N/16][Kpad/32][64 lanes][8] of the
// v_mfma_f32_16x16x32_f16 B operand (lane = n % 16 + 16 ((k / 8) % 4), element k % 8) —
// the layout of ftmi_highway_stack; else row-major [N][Kpad].
__global__ __launch_bounds__(256) void split_weights_f16_kernel(const float *__restrict__ w,
                                                                int64_t N, int64_t K, int64_t Kpad,
                                                                _Float16 *__restrict__ out,
                                                                float *__restrict__ colscale,
                                                                int frag) {
  __shared__ float red[4];
  const int64_t n = blockIdx.x;
  const float *row = w + n * K;
  float m = 0.f;
  for (int64_t k = threadIdx.x; k < K; k += 256) m = fmaxf(m, fabsf(row[k]));
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  int ex = 4;
  if (__builtin_isfinite(m) && m > 0.f) frexpf(m, &ex);  // m = f * 2^ex, f in [0.5, 1)
  const int e = ex - 4 > -100 ? ex - 4 : -100;           // 2^3 <= m * 2^-e < 2^4
  const int64_t plane = N * Kpad;
  for (int64_t k = threadIdx.x; k < Kpad; k += 256) {
    const float v = k < K ? ldexpf(row[k], -e) : 0.f;
    const _Float16 h = (_Float16)v;
    const _Float16 t = (_Float16)((v - (float)h) * H3_SCALE);
    const int64_t o = frag ? ((n >> 4) * (Kpad / 32) + (k >> 5)) * 512 + ((k >> 3) & 3) * 128 +
                                 (n & 15) * 8 + (k & 7)
                           : n * Kpad + k;
    out[o] = (_Float16)((float)h * H3_SCALE);
    out[plane + o] = t;
    out[2 * plane + o] = h;
  }
  if (threadIdx.x == 0) colscale[n] = ldexpf(1.f, e - 11);
}

// fp32 rows -> f16x3 split rows (include/ftmi.h): 4 channels per thread, range-checked
__global__ __launch_bounds__(256) void split_rows_kernel(const float *__restrict__ x,
                                                         int64_t x_stride, int64_t rows, int C,
                                                         float *__restrict__ y, int64_t y_stride,
                                                         unsigned *status) {
  const int C4 = C >> 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * C4) return;
  const int64_t r = i / C4;
  const int c = (int)(i - r * C4) * 4;
  const f32x4 v = *(const f32x4 *)(x + r * x_stride + c);
  f16x4 h, t;
  split2h(v, h, t);
  _Float16 *yr = (_Float16 *)(y + r * y_stride) + c;
  *(f16x4 *)yr = h;
  *(f16x4 *)(yr + C) = t;
  const float m = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
  if (!(m <= 65504.f) && status) atomicOr(status, 1u);
}

}  // namespace

extern "C" int64_t ftmi_split_weights_f16_bytes(int64_t N, int64_t K) {
  return split_block_bytes(N, K, 2);
}

static int split_f16(const float *w, int64_t N, int64_t K, void *out, int frag,
                     ftmi_stream_t stream) {
  if (!w || !out || N <= 0 || K <= 0) return FTMI_E_ARG;
  if (N > INT32_MAX || (frag && N % 16 != 0)) return FTMI_E_SHAPE;
  if (!ftmi_aligned16(out)) return FTMI_E_ALIGN;
  const int64_t Kpad = (K + X6_BK - 1) / X6_BK * X6_BK;
  hipLaunchKernelGGL(split_weights_f16_kernel, dim3((unsigned)N), dim3(256), 0, ftmi_hs(stream), w,
                     N, K, Kpad, (_Float16 *)out,
                     (float *)((char *)out + 3 * N * Kpad * 2), frag);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int ftmi_split_weights_f16(const float *w, int64_t N, int64_t K, void *out,
                                      ftmi_stream_t stream) {
  return split_f16(w, N, K, out, 0, stream);
}

extern "C" int ftmi_split_weights_f16_frag(const float *w, int64_t N, int64_t K, void *out,
                                           ftmi_stream_t stream) {
  return split_f16(w, N, K, out, 1, stream);
}

extern "C" int ftmi_split_rows(const float *x, int64_t x_stride, int64_t rows, int32_t C,
                               float *y, int64_t y_stride, uint32_t *status,
                               ftmi_stream_t stream) {
  if (!x || !y || rows < 0 || C <= 0) return FTMI_E_ARG;
  if (C % 4 || x_stride < C || y_stride < C) return FTMI_E_SHAPE;
  if (!ftmi_aligned16(x) || (x_stride & 3) || !ftmi_aligned16(y) || (y_stride & 3))
    return FTMI_E_ALIGN;
  if ((void *)x == (void *)y) return FTMI_E_ARG;  // rows are rewritten in another layout
  const int64_t n = rows * (C / 4);
  if (n == 0) return FTMI_OK;
  hipLaunchKernelGGL(split_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     ftmi_hs(stream), x, x_stride, rows, C, y, y_stride, status);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int ftmi_split_weights(const float *w, int64_t N, int64_t K, void *out,
                                  ftmi_stream_t stream) {
  if (!w || !out || N <= 0 || K <= 0) return FTMI_E_ARG;
  if (!ftmi_aligned16(out)) return FTMI_E_ALIGN;
  const int64_t Kpad = (K + X6_BK - 1) / X6_BK * X6_BK;
  const int64_t total = N * Kpad;
  const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(split_weights_kernel, dim3(blocks), dim3(256), 0, ftmi_hs(stream), w, N, K,
                     Kpad, (__bf16 *)out);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int64_t ftmi_split_weights_bytes(int64_t N, int64_t K) {
  return 3 * N * ((K + X6_BK - 1) / X6_BK * X6_BK) * 2;
}
