// Validation losses (the reference's evaluate() steps): masked / plain L1 (trainer/common.py:69-78,
// F.l1_loss), cross-entropy over rows of logits (F.cross_entropy) and the discretized
// mixture-of-logistics loss (utils/distribution.py:16-84).
//
// Every loss is a mean, computed as: a first launch in which each workgroup adds a fixed slice of
// the input in fp64, in a fixed order, and writes one fp64 partial to the caller's workspace; then
// a one-workgroup launch (ev_finish_kernel) that adds the partials in a fixed order (thread i takes
// partials i, i + EV_FIN_NT, ... in that order, the EV_FIN_NT sums meet in a fixed tree), divides
// and rounds to fp32 once.  No workgroup waits for another, nothing is added with atomics, and
// which slice a workgroup takes depends on the shape alone: the same input gives the same bits.
#include <math.h>

#include "common.h"

namespace {

constexpr int EV_FIN_NT = 1024;
constexpr int64_t EV_MAX_PARTS = (int64_t)1 << 22;  // workgroups of a first launch

// Sum of v over the block's NT threads: a fixed tree through s[NT].
template <int NT>
__device__ __forceinline__ double ev_block_sum(double v, double *s, int tid) {
  __syncthreads();  // s may still be read from the previous sum
  s[tid] = v;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  return s[0];
}

// out = (float)(sign * sum(parts) / denom).  denom: with lens, C * sum_b clamp(lens[b], 0, L) (an
// exact integer sum, 0 gives 0/0 = NaN like the reference); else denom_fixed.  iparts (optional):
// iout = their int32 sum.
__global__ __launch_bounds__(EV_FIN_NT) void ev_finish_kernel(
    const double *__restrict__ parts, int nparts, const int32_t *__restrict__ iparts,
    const int32_t *__restrict__ lens, int B, int L, int C, double denom_fixed, double sign,
    float *__restrict__ out, int32_t *__restrict__ iout) {
  __shared__ double s_red[EV_FIN_NT];
  __shared__ long long s_cnt[EV_FIN_NT];
  const int tid = threadIdx.x;
  double acc = 0.0;
  long long cnt = 0;
  for (int i = tid; i < nparts; i += EV_FIN_NT) acc += parts[i];
  if (iparts)
    for (int i = tid; i < nparts; i += EV_FIN_NT) cnt += iparts[i];
  const double sum = ev_block_sum<EV_FIN_NT>(acc, s_red, tid);
  if (iparts) {
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int o = EV_FIN_NT / 2; o > 0; o >>= 1) {
      if (tid < o) s_cnt[tid] += s_cnt[tid + o];
      __syncthreads();
    }
    if (tid == 0) iout[0] = (int32_t)(s_cnt[0] > 0x7fffffffLL ? 0x7fffffffLL : s_cnt[0]);
    __syncthreads();
  }
  double denom = denom_fixed;
  if (lens) {
    long long n = 0;
    for (int b = tid; b < B; b += EV_FIN_NT) n += min(max(lens[b], 0), L);
    s_cnt[tid] = n;
    __syncthreads();
    for (int o = EV_FIN_NT / 2; o > 0; o >>= 1) {
      if (tid < o) s_cnt[tid] += s_cnt[tid + o];
      __syncthreads();
    }
    denom = (double)C * (double)s_cnt[0];
  }
  if (tid == 0) out[0] = (float)(sign * sum / denom);
}

// ---------------------------------------------------------------------------------------
// L1.  A workgroup owns item b = blockIdx.x / tiles and frames [t0, t0 + 32), and walks the
// channels in tiles of 32.  Both operands pass through LDS, each loaded along whichever of its
// axes has unit stride (x is often a transposed view while the target is not), then thread
// (c = tid / 32 + 8 k, t = tid % 32) adds |x - target| of its four elements: the order of the
// additions does not depend on either layout.  Nothing at t >= n_b or c >= C is loaded.
constexpr int L1_NT = 256;
constexpr int L1_TILE = 32;

__device__ __forceinline__ void l1_load_tile(const float *__restrict__ p, int64_t s_c, int64_t s_t,
                                             int c0, int nc, int t0, int nt, float (*s)[L1_TILE + 1],
                                             int tid) {
  const bool frame_major = s_t == 1;
#pragma unroll
  for (int e = tid; e < L1_TILE * L1_TILE; e += L1_NT) {
    const int lo = e & (L1_TILE - 1), hi = e >> 5;
    const int cl = frame_major ? hi : lo, tl = frame_major ? lo : hi;
    if (cl < nc && tl < nt) s[cl][tl] = p[(int64_t)(c0 + cl) * s_c + (int64_t)(t0 + tl) * s_t];
  }
}

__global__ __launch_bounds__(L1_NT) void l1_partial_kernel(
    const float *__restrict__ x, int64_t xs_b, int64_t xs_c, int64_t xs_t,
    const float *__restrict__ tg, int64_t ts_b, int64_t ts_c, int64_t ts_t, int C, int L, int tiles,
    const int32_t *__restrict__ lens, double *__restrict__ parts) {
  __shared__ float s_x[L1_TILE][L1_TILE + 1];
  __shared__ float s_t[L1_TILE][L1_TILE + 1];
  __shared__ double s_red[L1_NT];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * L1_TILE;
  const int n = lens ? min(max(lens[b], 0), L) : L;
  const int nt = min(n - t0, L1_TILE);  // <= 0: this tile is all padding (uniform over the block)
  double acc = 0.0;
  if (nt > 0) {
    const float *xb = x + (int64_t)b * xs_b, *tb = tg + (int64_t)b * ts_b;
    const int tl = tid & (L1_TILE - 1), cq = tid >> 5;
    for (int c0 = 0; c0 < C; c0 += L1_TILE) {
      const int nc = min(C - c0, L1_TILE);
      __syncthreads();
      l1_load_tile(xb, xs_c, xs_t, c0, nc, t0, nt, s_x, tid);
      l1_load_tile(tb, ts_c, ts_t, c0, nc, t0, nt, s_t, tid);
      __syncthreads();
      if (tl < nt) {
#pragma unroll
        for (int k = 0; k < L1_TILE * L1_TILE / L1_NT; ++k) {
          const int cl = cq + k * (L1_NT / L1_TILE);
          if (cl < nc) acc += fabs((double)s_x[cl][tl] - (double)s_t[cl][tl]);
        }
      }
    }
  }
  const double sum = ev_block_sum<L1_NT>(acc, s_red, tid);
  if (tid == 0) parts[blockIdx.x] = sum;
}

// ---------------------------------------------------------------------------------------
// Cross-entropy.  A wave per row, CE_RPW rows per wave one after the other, CE_NW waves per
// workgroup: the workgroup's partial is the sum over its CE_NW * CE_RPW rows.  Lane i reads
// columns i, i + 64, ...; the row maximum is exact in fp32, the sum of exp(x - m) is fp64 and
// meets across the lanes in a butterfly (every lane ends with the same bits).
constexpr int CE_NW = 4;
constexpr int CE_RPW = 4;
constexpr int CE_ROWS = CE_NW * CE_RPW;

__global__ __launch_bounds__(CE_NW * 64) void ce_partial_kernel(
    const float *__restrict__ logits, int64_t ld, int64_t rows, int C,
    const int32_t *__restrict__ target, double *__restrict__ parts, int32_t *__restrict__ bad_parts) {
  __shared__ double s_w[CE_NW];
  __shared__ int s_b[CE_NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  int bad = 0;
  for (int k = 0; k < CE_RPW; ++k) {
    const int64_t r = (int64_t)blockIdx.x * CE_ROWS + wave * CE_RPW + k;
    if (r >= rows) break;  // uniform over the wave
    const float *row = logits + r * ld;
    float m = -INFINITY;
    for (int j = lane; j < C; j += 64) m = fmaxf(m, row[j]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    double s = 0.0;
    for (int j = lane; j < C; j += 64) s += exp((double)row[j] - (double)m);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const int t = target[r];
    if (t >= 0 && t < C)
      acc += (double)m + log(s) - (double)row[t];
    else
      bad += 1;
  }
  if (lane == 0) { s_w[wave] = acc; s_b[wave] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.0;
    int nb = 0;
    for (int w = 0; w < CE_NW; ++w) { sum += s_w[w]; nb += s_b[w]; }
    parts[blockIdx.x] = sum;
    bad_parts[blockIdx.x] = nb;
  }
}

// ---------------------------------------------------------------------------------------
// Discretized mixture of logistics (utils/distribution.py:16-84), a thread per row, every term in
// fp64.  The reference blends its branches with 0/1 masks; for finite operands a select gives the
// same value, and here a non-finite value of a branch that is not taken reaches no result.
constexpr int MOL_NT = 128;
constexpr int MOL_KMAX = 32;

__device__ __forceinline__ double ev_softplus(double v) { return v > 20.0 ? v : log1p(exp(v)); }
__device__ __forceinline__ double ev_sigmoid(double v) { return 1.0 / (1.0 + exp(-v)); }

__global__ __launch_bounds__(MOL_NT) void mol_partial_kernel(
    const float *__restrict__ y_hat, int64_t ld, int64_t rows, int K, const float *__restrict__ y,
    double half_bin, double log_half_classes, double log_scale_min, double *__restrict__ parts,
    float *__restrict__ per_sample) {
  __shared__ double s_lp[MOL_KMAX][MOL_NT];
  __shared__ double s_red[MOL_NT];
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * MOL_NT + tid;
  double lse = 0.0;
  if (r < rows) {
    const float *row = y_hat + r * ld;
    const float yf = y[r];
    const double yd = (double)yf;
    // log_softmax of the mixture logits
    double lm = -INFINITY;
    for (int k = 0; k < K; ++k) lm = fmax(lm, (double)row[k]);
    double ls = 0.0;
    for (int k = 0; k < K; ++k) ls += exp((double)row[k] - lm);
    const double lnorm = lm + log(ls);
    const bool low = yf < -0.999f, high = yf > 0.999f;  // fp32 compares, like torch's
    double pm = -INFINITY;
    for (int k = 0; k < K; ++k) {
      const double mean = (double)row[K + k];
      const double log_scale = fmax((double)row[2 * K + k], log_scale_min);
      const double centered = yd - mean;
      const double inv_stdv = exp(-log_scale);
      const double plus_in = __dmul_rn(inv_stdv, centered + half_bin);
      const double min_in = __dmul_rn(inv_stdv, centered - half_bin);
      const double mid_in = __dmul_rn(inv_stdv, centered);
      double lp;
      if (low) {
        lp = plus_in - ev_softplus(plus_in);
      } else if (high) {
        lp = -ev_softplus(min_in);
      } else {
        const double cdf_delta = ev_sigmoid(plus_in) - ev_sigmoid(min_in);
        if (cdf_delta > 1e-5)
          lp = log(fmax(cdf_delta, 1e-12));
        else
          lp = (mid_in - log_scale - 2.0 * ev_softplus(mid_in)) - log_half_classes;
      }
      lp += (double)row[k] - lnorm;
      s_lp[k][tid] = lp;
      pm = fmax(pm, lp);
    }
    double ps = 0.0;
    for (int k = 0; k < K; ++k) ps += exp(s_lp[k][tid] - pm);
    lse = pm + log(ps);
    if (per_sample) per_sample[r] = (float)(-lse);
  }
  const double sum = ev_block_sum<MOL_NT>(lse, s_red, tid);
  if (tid == 0) parts[blockIdx.x] = sum;
}

inline int64_t l1_tiles(int32_t L) { return ((int64_t)L + L1_TILE - 1) / L1_TILE; }
inline int64_t ce_blocks(int64_t rows) { return (rows + CE_ROWS - 1) / CE_ROWS; }
inline int64_t mol_blocks(int64_t rows) { return (rows + MOL_NT - 1) / MOL_NT; }

// a (C, L) plane is either frame-major (unit frame stride, channel stride >= L) or channel-major
// (unit channel stride, frame stride >= C)
inline bool l1_strides_ok(int64_t s_b, int64_t s_c, int64_t s_t, int32_t C, int32_t L) {
  if (s_b < 0) return false;
  return (s_t == 1 && s_c >= L) || (s_c == 1 && s_t >= C);
}

}  // namespace

extern "C" int64_t ftmi_l1_loss_workspace_bytes(int32_t B, int32_t C, int32_t L) {
  if (B <= 0 || C <= 0 || L <= 0) return 0;
  const int64_t n = (int64_t)B * l1_tiles(L);
  return n <= EV_MAX_PARTS ? n * 8 : 0;
}

extern "C" int ftmi_l1_loss(const float *x, int64_t xs_item, int64_t xs_chan, int64_t xs_frame,
                            const float *target, int64_t ts_item, int64_t ts_chan, int64_t ts_frame,
                            int32_t B, int32_t C, int32_t L, const int32_t *lens, float *out,
                            void *workspace, ftmi_stream_t stream) {
  if (!x || !target || !out || !workspace) return FTMI_E_ARG;
  if (B <= 0 || C <= 0 || L <= 0) return FTMI_E_ARG;
  if (!l1_strides_ok(xs_item, xs_chan, xs_frame, C, L) ||
      !l1_strides_ok(ts_item, ts_chan, ts_frame, C, L))
    return FTMI_E_SHAPE;
  const int64_t tiles = l1_tiles(L), nparts = (int64_t)B * tiles;
  if (nparts > EV_MAX_PARTS) return FTMI_E_UNSUPPORTED;
  if ((((uintptr_t)x | (uintptr_t)target | (uintptr_t)lens | (uintptr_t)out) & 3u) ||
      !ftmi_aligned16(workspace))
    return FTMI_E_ALIGN;
  double *parts = (double *)workspace;
  hipLaunchKernelGGL(l1_partial_kernel, dim3((unsigned)nparts), dim3(L1_NT), 0, ftmi_hs(stream), x,
                     xs_item, xs_chan, xs_frame, target, ts_item, ts_chan, ts_frame, C, L,
                     (int)tiles, lens, parts);
  FTMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(ev_finish_kernel, dim3(1), dim3(EV_FIN_NT), 0, ftmi_hs(stream), parts,
                     (int)nparts, (const int32_t *)nullptr, lens, B, L, C,
                     (double)B * (double)C * (double)L, 1.0, out, (int32_t *)nullptr);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int64_t ftmi_cross_entropy_workspace_bytes(int64_t rows, int32_t C) {
  if (rows <= 0 || C <= 0 || C > 65536) return 0;
  const int64_t n = ce_blocks(rows);
  return n <= EV_MAX_PARTS ? n * 12 : 0;  // an fp64 partial and an int32 label count each
}

extern "C" int ftmi_cross_entropy(const float *logits, int64_t ld, int64_t rows, int32_t C,
                                  const int32_t *target, float *out, int32_t *bad_out,
                                  void *workspace, ftmi_stream_t stream) {
  if (!logits || !target || !out || !bad_out || !workspace) return FTMI_E_ARG;
  if (rows <= 0 || C <= 0) return FTMI_E_ARG;
  if (ld < C) return FTMI_E_SHAPE;
  const int64_t nparts = ce_blocks(rows);
  if (C > 65536 || nparts > EV_MAX_PARTS) return FTMI_E_UNSUPPORTED;
  if ((((uintptr_t)logits | (uintptr_t)target | (uintptr_t)out | (uintptr_t)bad_out) & 3u) ||
      !ftmi_aligned16(workspace))
    return FTMI_E_ALIGN;
  double *parts = (double *)workspace;
  int32_t *bad_parts = (int32_t *)(parts + nparts);
  hipLaunchKernelGGL(ce_partial_kernel, dim3((unsigned)nparts), dim3(CE_NW * 64), 0, ftmi_hs(stream),
                     logits, ld, rows, C, target, parts, bad_parts);
  FTMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(ev_finish_kernel, dim3(1), dim3(EV_FIN_NT), 0, ftmi_hs(stream), parts,
                     (int)nparts, (const int32_t *)bad_parts, (const int32_t *)nullptr, 0, 0, 0,
                     (double)rows, 1.0, out, bad_out);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int64_t ftmi_mol_loss_workspace_bytes(int64_t rows, int32_t K) {
  if (rows <= 0 || K <= 0 || K > MOL_KMAX) return 0;
  const int64_t n = mol_blocks(rows);
  return n <= EV_MAX_PARTS ? n * 8 : 0;
}

extern "C" int ftmi_mol_loss(const float *y_hat, int64_t ld, int64_t rows, int32_t channels,
                             const float *y, double num_classes, double log_scale_min, float *out,
                             float *per_sample, void *workspace, ftmi_stream_t stream) {
  if (!y_hat || !y || !out || !workspace) return FTMI_E_ARG;
  if (rows <= 0 || channels <= 0 || !(num_classes > 1.0) || log_scale_min != log_scale_min)
    return FTMI_E_ARG;
  if (channels % 3 != 0 || channels / 3 > MOL_KMAX) return FTMI_E_UNSUPPORTED;
  if (ld < channels) return FTMI_E_SHAPE;
  const int64_t nparts = mol_blocks(rows);
  if (nparts > EV_MAX_PARTS) return FTMI_E_UNSUPPORTED;
  if ((((uintptr_t)y_hat | (uintptr_t)y | (uintptr_t)out | (uintptr_t)per_sample) & 3u) ||
      !ftmi_aligned16(workspace))
    return FTMI_E_ALIGN;
  double *parts = (double *)workspace;
  hipLaunchKernelGGL(mol_partial_kernel, dim3((unsigned)nparts), dim3(MOL_NT), 0, ftmi_hs(stream),
                     y_hat, ld, rows, channels / 3, y, 1.0 / (num_classes - 1.0),
                     log((num_classes - 1.0) / 2.0), log_scale_min, parts, per_sample);
  FTMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(ev_finish_kernel, dim3(1), dim3(EV_FIN_NT), 0, ftmi_hs(stream), parts,
                     (int)nparts, (const int32_t *)nullptr, (const int32_t *)nullptr, 0, 0, 0,
                     (double)rows, -1.0, out, (int32_t *)nullptr);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}
