// Audio preparation of preprocess.py (Preprocessor._convert_file :51-91) on gfx950: the
// start / end silence trim (utils/dsp.py:112-113 -> librosa 0.7.2 effects.trim), the peak
// rule and the vocoder's label sequence (utils/dsp.py:143-153).  The log-mel of the prepared
// rows is ftmi_mel_spectrogram (dsp.hip).
//
// Four streaming kernels, none of which waits for another workgroup:
//   frame_power   mean square of every centred, reflect-padded frame: fp64 sums in a fixed
//                 order, one rounding to float32
//   trim_bounds   per item: the loudest frame, the fp64 dB test, first / last frame over it
//   peak_abs      max |y| over an item's [start, end) (a maximum has no order: the integer
//                 atomic max over the bit patterns of |y| gives the same bits on every call)
//   prepare       the [start, end) samples left-aligned, divided by the peak where the rule
//                 says so, zero-filled to the row; the int64 labels; the new lengths
#include <math.h>

#include "common.h"

// the label arithmetic restates numpy's: every float32 / float64 operation rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int PREP_NT = 256;
constexpr int PREP_WAVES = PREP_NT / 64;
constexpr int FP_TF = 32;    // frames per workgroup
constexpr int FP_MAXR = 64;  // most hop blocks per frame on the block-sum path
constexpr int PREP_CHUNK = 4096;  // samples per workgroup of the element-wise kernels

__device__ __forceinline__ int64_t item_len(const int32_t *lengths, int b, int64_t L) {
  if (!lengths) return L;
  const int64_t v = lengths[b];
  return v < 0 ? 0 : (v > L ? L : v);
}

// Frame f covers padded samples [f hop, f hop + frame_length), padded index k being sample
// reflect(k - frame_length / 2).  A tile of FP_TF frames is cut into segments of seg_len
// samples that start hop apart: seg_len = hop and R = frame_length / hop segments per frame
// when hop divides the frame (each sample squared once per tile, R - 1 segments shared with
// the next tile), or seg_len = frame_length and R = 1 otherwise.  A wave owns a segment: lane
// l adds samples l, l + 64, ... in that order, the 64 sums meet in a fixed tree, and a frame
// adds its R segments in ascending order: the bits depend on the item's samples alone.
__global__ __launch_bounds__(PREP_NT) void frame_power_kernel(
    const float *__restrict__ y, int64_t y_stride, int64_t L, const int32_t *__restrict__ lengths,
    int frame_length, int hop, int F, int seg_len, int R, float *__restrict__ power) {
  __shared__ double s_seg[FP_TF + FP_MAXR];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.y, f0 = blockIdx.x * FP_TF;
  const int64_t Lb = item_len(lengths, b, L);
  const int64_t Fb = min((int64_t)F, 1 + Lb / hop);
  const int nf = min(FP_TF, F - f0);                             // frames of the tile in the row
  const int nv = (int)max((int64_t)0, min((int64_t)nf, Fb - f0));  // ... that belong to the item
  const float *yb = y + (int64_t)b * y_stride;
  if (nv > 0) {  // uniform over the workgroup
    const int nseg = nv + R - 1;
    for (int s = wave; s < nseg; s += PREP_WAVES) {
      const int64_t j0 = (int64_t)(f0 + s) * hop - frame_length / 2;
      double acc = 0.0;
      if (j0 >= 0 && j0 + seg_len <= Lb) {
        for (int i = lane; i < seg_len; i += 64) {
          const double v = (double)yb[j0 + i];
          acc += v * v;
        }
      } else {
        for (int i = lane; i < seg_len; i += 64) {
          const double v = (double)yb[reflect_index(j0 + i, Lb)];
          acc += v * v;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
      if (lane == 0) s_seg[s] = acc;
    }
    __syncthreads();
  }
  for (int f = tid; f < nf; f += PREP_NT) {
    float out = 0.0f;
    if (f < nv) {
      double sum = 0.0;
      for (int r = 0; r < R; ++r) sum += s_seg[f + r];
      out = (float)(sum / (double)frame_length);
    }
    power[(int64_t)b * F + f0 + f] = out;
  }
}

// One workgroup per item.  librosa core.power_to_db(ref=np.max, amin=1e-10, top_db=None) of
// the item's own frames, in fp64 from the float32 powers, then `> -top_db`.
__global__ __launch_bounds__(PREP_NT) void trim_bounds_kernel(
    const float *__restrict__ power, int F, int64_t L, const int32_t *__restrict__ lengths, int hop,
    double top_db, int32_t *__restrict__ bounds) {
  __shared__ float s_max[PREP_NT];
  __shared__ int s_lo[PREP_NT], s_hi[PREP_NT];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int64_t Lb = item_len(lengths, b, L);
  const int Fb = (int)min((int64_t)F, 1 + Lb / hop);
  const float *pb = power + (int64_t)b * F;
  float m = 0.0f;  // powers are >= 0
  for (int f = tid; f < Fb; f += PREP_NT) m = fmaxf(m, pb[f]);
  s_max[tid] = m;
  __syncthreads();
  for (int o = PREP_NT / 2; o > 0; o >>= 1) {
    if (tid < o) s_max[tid] = fmaxf(s_max[tid], s_max[tid + o]);
    __syncthreads();
  }
  const double ref = 10.0 * log10(fmax(1e-10, (double)s_max[0]));
  int lo = F, hi = -1;
  for (int f = tid; f < Fb; f += PREP_NT) {
    const double db = 10.0 * log10(fmax(1e-10, (double)pb[f])) - ref;
    if (db > -top_db) {
      lo = min(lo, f);
      hi = max(hi, f);
    }
  }
  s_lo[tid] = lo, s_hi[tid] = hi;
  __syncthreads();
  for (int o = PREP_NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s_lo[tid] = min(s_lo[tid], s_lo[tid + o]);
      s_hi[tid] = max(s_hi[tid], s_hi[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool any = s_hi[0] >= 0;
    const int64_t start = any ? (int64_t)s_lo[0] * hop : 0;
    const int64_t end = any ? min(Lb, ((int64_t)s_hi[0] + 1) * hop) : 0;
    // first <= Lb / hop, so start <= end <= Lb; a last frame that starts at the item's end
    // (L % hop == 0) and is alone over the threshold gives the empty slice [L, L), as the
    // reference does
    bounds[2 * b] = (int32_t)start;
    bounds[2 * b + 1] = (int32_t)end;
  }
}

// [start, end) of item b clamped into the row (never trusts the device values for addressing)
__device__ __forceinline__ void item_bounds(const int32_t *bounds, int b, int64_t L, int64_t &s,
                                            int64_t &n) {
  int64_t st = bounds[2 * b], en = bounds[2 * b + 1];
  st = st < 0 ? 0 : (st > L ? L : st);
  en = en < st ? st : (en > L ? L : en);
  s = st, n = en - st;
}

__global__ __launch_bounds__(PREP_NT) void peak_abs_kernel(
    const float *__restrict__ y, int64_t y_stride, int64_t L, const int32_t *__restrict__ bounds,
    unsigned int *__restrict__ peak_bits) {
  __shared__ unsigned int s_m[PREP_NT];
  const int tid = threadIdx.x, b = blockIdx.y;
  int64_t st, n;
  item_bounds(bounds, b, L, st, n);
  const int64_t i0 = (int64_t)blockIdx.x * PREP_CHUNK;
  if (i0 >= n) return;  // uniform over the workgroup
  const int64_t i1 = min(n, i0 + PREP_CHUNK);
  const float *yb = y + (int64_t)b * y_stride + st;
  unsigned int m = 0;
  for (int64_t i = i0 + tid; i < i1; i += PREP_NT) m = max(m, __float_as_uint(fabsf(yb[i])));
  s_m[tid] = m;
  __syncthreads();
  for (int o = PREP_NT / 2; o > 0; o >>= 1) {
    if (tid < o) s_m[tid] = max(s_m[tid], s_m[tid + o]);
    __syncthreads();
  }
  // |y| >= 0: IEEE order is the order of the bit patterns; NaN sorts above everything
  if (tid == 0) atomicMax(peak_bits + b, s_m[0]);
}

struct PrepParams {
  const float *y;
  int64_t y_stride, L;
  const int32_t *bounds;
  const float *peak;
  int peak_norm, mu_law, bits;
  double log1p_mu;  // log(1 + mu), mu = 2^bits - 1
  float *out;
  int64_t out_stride;
  int64_t *quant;
  int64_t q_stride;
  int32_t *new_len;
};

__global__ __launch_bounds__(PREP_NT) void prepare_kernel(const PrepParams p) {
  const int tid = threadIdx.x, b = blockIdx.y;
  int64_t st, n;
  item_bounds(p.bounds, b, p.L, st, n);
  if (blockIdx.x == 0 && tid == 0) p.new_len[b] = (int32_t)n;
  const float peak = p.peak[b];
  // the reference divides whenever the rule holds; an all-zero item (peak 0) stays unscaled
  const bool scale = (p.peak_norm || peak > 1.0f) && peak > 0.0f;
  const float *yb = p.y + (int64_t)b * p.y_stride + st;
  float *ob = p.out + (int64_t)b * p.out_stride;
  int64_t *qb = p.quant ? p.quant + (int64_t)b * p.q_stride : nullptr;
  const double mu = (double)((1 << p.bits) - 1);
  const float muf = (float)((1 << p.bits) - 1);
  const int64_t i0 = (int64_t)blockIdx.x * PREP_CHUNK, i1 = min(p.L, i0 + PREP_CHUNK);
  for (int64_t i = i0 + tid; i < i1; i += PREP_NT) {
    float v = 0.0f;
    int64_t q = 0;
    if (i < n) {
      v = yb[i];
      if (scale) v = __fdiv_rn(v, peak);
      if (qb) {
        if (p.mu_law) {
          // DSP.encode_mu_law on float64(v): sign * log(1 + mu |x|) / log(1 + mu), then
          // floor((fx + 1) / 2 * mu + 0.5)
          const double x = (double)v;
          const double sg = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0);
          const double fx = sg * log(1.0 + mu * fabs(x)) / p.log1p_mu;
          q = (int64_t)floor((fx + 1.0) / 2.0 * mu + 0.5);
        } else {
          // DSP.float_2_label on float32: (x + 1) * (2^bits - 1) / 2, clipped, truncated
          float t = v + 1.0f;
          t = t * muf;
          t = __fdiv_rn(t, 2.0f);
          t = fminf(fmaxf(t, 0.0f), muf);
          q = (int64_t)t;
        }
      }
    }
    ob[i] = v;
    if (qb) qb[i] = q;
  }
}

int check_rows(const float *y, int64_t y_stride, int32_t B, int64_t L) {
  if (!y || B <= 0 || L < 2) return FTMI_E_ARG;
  if (L > 0x7fffffffLL || y_stride < L) return FTMI_E_SHAPE;
  if (B > 65535) return FTMI_E_UNSUPPORTED;
  return FTMI_OK;
}

}  // namespace

extern "C" int ftmi_frame_power(const float *y, int64_t y_stride, int32_t B, int64_t L,
                                const int32_t *lengths, int32_t frame_length, int32_t hop,
                                int32_t F, float *power, ftmi_stream_t stream) {
  if (!power) return FTMI_E_ARG;
  if (int rc = check_rows(y, y_stride, B, L)) return rc;
  if (frame_length <= 0 || (frame_length & 1) || hop < 1) return FTMI_E_ARG;
  if (F <= 0 || (int64_t)F > 1 + L / hop) return FTMI_E_SHAPE;
  int seg_len = frame_length, R = 1;
  if (frame_length % hop == 0 && frame_length / hop <= FP_MAXR)
    seg_len = hop, R = frame_length / hop;
  dim3 grid((F + FP_TF - 1) / FP_TF, B);
  hipLaunchKernelGGL(frame_power_kernel, grid, dim3(PREP_NT), 0, ftmi_hs(stream), y, y_stride, L,
                     lengths, frame_length, hop, F, seg_len, R, power);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int ftmi_trim_bounds(const float *power, int32_t B, int32_t F, int64_t L,
                                const int32_t *lengths, int32_t hop, double top_db,
                                int32_t *bounds, ftmi_stream_t stream) {
  if (!power || !bounds || B <= 0 || F <= 0 || L < 2 || hop < 1) return FTMI_E_ARG;
  if (L > 0x7fffffffLL || (int64_t)F > 1 + L / hop) return FTMI_E_SHAPE;
  if (!(top_db == top_db)) return FTMI_E_ARG;
  hipLaunchKernelGGL(trim_bounds_kernel, dim3(B), dim3(PREP_NT), 0, ftmi_hs(stream), power, F, L,
                     lengths, hop, top_db, bounds);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int ftmi_peak_abs(const float *y, int64_t y_stride, int32_t B, int64_t L,
                             const int32_t *bounds, float *peak, ftmi_stream_t stream) {
  if (!bounds || !peak) return FTMI_E_ARG;
  if (int rc = check_rows(y, y_stride, B, L)) return rc;
  hipError_t e = hipMemsetAsync(peak, 0, (size_t)B * sizeof(float), ftmi_hs(stream));
  if (e != hipSuccess) return (int)e;
  dim3 grid((unsigned)((L + PREP_CHUNK - 1) / PREP_CHUNK), B);
  hipLaunchKernelGGL(peak_abs_kernel, grid, dim3(PREP_NT), 0, ftmi_hs(stream), y, y_stride, L,
                     bounds, (unsigned int *)peak);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int ftmi_prepare_audio(const float *y, int64_t y_stride, int32_t B, int64_t L,
                                  const int32_t *bounds, const float *peak, int32_t peak_norm,
                                  int32_t mu_law, int32_t bits, float *out, int64_t out_stride,
                                  int64_t *quant, int64_t quant_stride, int32_t *new_len,
                                  ftmi_stream_t stream) {
  if (!bounds || !peak || !out || !new_len) return FTMI_E_ARG;
  if (int rc = check_rows(y, y_stride, B, L)) return rc;
  if (bits < 1 || bits > 16) return FTMI_E_UNSUPPORTED;
  if (out_stride < L || (quant && quant_stride < L)) return FTMI_E_SHAPE;
  if ((const void *)out == (const void *)y) return FTMI_E_ARG;  // rows move left: not in place
  PrepParams p = {};
  p.y = y, p.y_stride = y_stride, p.L = L, p.bounds = bounds, p.peak = peak;
  p.peak_norm = peak_norm != 0, p.mu_law = mu_law != 0, p.bits = bits;
  p.log1p_mu = log(1.0 + (double)((1 << bits) - 1));
  p.out = out, p.out_stride = out_stride, p.quant = quant, p.q_stride = quant_stride;
  p.new_len = new_len;
  dim3 grid((unsigned)((L + PREP_CHUNK - 1) / PREP_CHUNK), B);
  hipLaunchKernelGGL(prepare_kernel, grid, dim3(PREP_NT), 0, ftmi_hs(stream), p);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}
