// Conv bank of an EMBEDDED sequence as a table gather (ftmi_embed_bank).
//
// A convolution of embedding rows is linear in them, so for kernel size k, tap j and symbol s
// the product W_k[:, :, j] . E[s] is a constant of the weights: Tab[s][k][j][:].  The bank
// before its ReLU is then a sum of k gathered rows per (token, kernel size),
//   y_k[b, t, :] = sum_{j < k, 0 <= t + j - k/2 < T} Tab[ids[b, t + j - k/2]][k][j][:]
// summed in tap order in fp32 (one fixed order, no atomics: launches are bit-identical).
//
// Work layout: a wave owns EB_ROWS consecutive (b, t) rows of one PAIR of kernel sizes
// (kmin + i, kmax - i) and one 256-column panel: a lane holds 4 columns, so each gathered row
// and each stored row segment is 1 KB contiguous per wave (512 B + 512 B as split rows).  All
// taps of a row — kmin + kmax of them for every pair, so the pairs carry equal work — are
// issued before the first add.  Workgroup w takes pair w % slices: with the bank's 8 pairs and
// round-robin dispatch over the 8 XCDs, every workgroup of an XCD gathers from one pair's
// 1/8 of the table (2.35 MB for the 16-kernel bank of 135 symbols), which its 4 MB L2 holds.
// Placement only changes where the rows are served from, never a result.
// The maxpool(2, 1) needs the previous row: a wave walks its rows in order and keeps it in
// registers; the row before its first is recomputed (1 / EB_ROWS extra gathers).
#include "common.h"

namespace {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef decltype(__builtin_amdgcn_make_buffer_rsrc((void *)nullptr, (short)0, 0, 0)) EbRsrc;

constexpr int EB_ROWS = 16;   // rows per wave
constexpr int EB_WAVES = 4;   // waves per workgroup
constexpr int EB_KMAX = 16;   // largest kernel size: EB_ROWS + 1 + EB_KMAX ids fit a wave's lanes
constexpr int EB_PANEL = 256; // columns per wave (4 per lane)
constexpr float EB_TAIL = 2048.f;  // 2^11: the tail scale of f16x3 split rows (include/ftmi.h)

struct EbParams {
  const int64_t *ids;
  int T, M;           // M = B * T rows
  const float *tab;   // [S][taps][Cout]
  int S, taps, Cout;
  int kmin, kmax, slices;
  const float *scale, *shift;  // [G * Cout]
  float *y;
  int64_t y_stride;
  int pool, split;
  unsigned *status;
};

__device__ __forceinline__ f32x4 eb_max4(f32x4 a, f32x4 b) {
  return (f32x4){fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)};
}

// taps of the kernel sizes below k (the table's tap order: k = kmin.., j = 0..k-1)
__device__ __forceinline__ int eb_tap_base(int k, int kmin) {
  return (k * (k - 1) - kmin * (kmin - 1)) / 2;
}

// One kernel size's operands of a run of rows.  idv: lane l holds the id of row wlo + l, or -1
// where that row is outside [0, M) or its id outside [0, S).
template <int K>
struct EbGroup {
  f32x4 v[K];
  bool ok[K];
  f32x4 sc, sh, prev;
  unsigned tap0;  // first tap of this kernel size in a symbol's table rows

  __device__ __forceinline__ void init(const EbParams &p, int k, unsigned col) {
    const int g = k - p.kmin;
    sc = *(const f32x4 *)(p.scale + (int64_t)g * p.Cout + col);
    sh = *(const f32x4 *)(p.shift + (int64_t)g * p.Cout + col);
    prev = (f32x4){0.f, 0.f, 0.f, 0.f};
    tap0 = (unsigned)eb_tap_base(k, p.kmin);
  }
  // issue the K gathers of row r (position t of its sequence): buffer loads, the row's byte
  // offset wave-uniform (a scalar register), the lane's columns (voff bytes) the only VGPR
  __device__ __forceinline__ void load(const EbParams &p, EbRsrc rs, unsigned voff, int idv,
                                       int wlo, int r, int t) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int d = j - K / 2;
      const int id = __builtin_amdgcn_readlane(idv, r + d - wlo);
      ok[j] = (unsigned)(t + d) < (unsigned)p.T && id >= 0;
      const unsigned row = (unsigned)(ok[j] ? id : 0) * (unsigned)p.taps + tap0 + j;
      v[j] = __builtin_bit_cast(
          f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, row * (unsigned)p.Cout * 4u, 0));
    }
  }
  // sum in tap order, ReLU, BN; returns the row's (pooled) output and keeps it as `prev`
  __device__ __forceinline__ f32x4 finish(bool pool_prev) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < K; ++j) acc += ok[j] ? v[j] : (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 o = eb_max4(acc, (f32x4){0.f, 0.f, 0.f, 0.f});
    o = o * sc + sh;
    const f32x4 out = pool_prev ? eb_max4(prev, o) : o;
    prev = o;
    return out;
  }
  // whether the row just finished holds a NaN before the pool (whose fmaxf would drop it)
  __device__ __forceinline__ bool nan() const {
    return prev.x != prev.x || prev.y != prev.y || prev.z != prev.z || prev.w != prev.w;
  }
};
template <>
struct EbGroup<0> {
  __device__ __forceinline__ void init(const EbParams &, int, unsigned) {}
  __device__ __forceinline__ void load(const EbParams &, EbRsrc, unsigned, int, int, int, int) {}
  __device__ __forceinline__ f32x4 finish(bool) { return (f32x4){0.f, 0.f, 0.f, 0.f}; }
  __device__ __forceinline__ bool nan() const { return false; }
};

// stores one row segment; true if it went out as split rows with a value beyond the f16 range
// or not a number (tested per value: fmaxf would drop a NaN)
__device__ __forceinline__ bool eb_store(const EbParams &p, int r, int ycol, f32x4 o) {
  if (p.split) {
    const f16x4 h = __builtin_convertvector(o, f16x4);
    const f16x4 t =
        __builtin_convertvector((o - __builtin_convertvector(h, f32x4)) * EB_TAIL, f16x4);
    _Float16 *yr = (_Float16 *)(p.y + (int64_t)r * p.y_stride) + ycol;
    *(f16x4 *)yr = h;
    *(f16x4 *)(yr + (int64_t)(p.kmax - p.kmin + 1) * p.Cout) = t;
    return !(fabsf(o.x) <= 65504.f) || !(fabsf(o.y) <= 65504.f) || !(fabsf(o.z) <= 65504.f) ||
           !(fabsf(o.w) <= 65504.f);
  }
  *(f32x4 *)(p.y + (int64_t)r * p.y_stride + ycol) = o;
  return false;
}

// rows [r0, r1) of kernel sizes KA (= ka) and, if KB > 0, KB (= kb)
template <int KA, int KB>
__device__ __forceinline__ void eb_run(const EbParams &p, int idv, int wlo, int r0, int r1,
                                       int ka, int kb, int col) {
  EbGroup<KA> A;
  EbGroup<KB> Bg;
  A.init(p, ka, col);
  Bg.init(p, kb, col);
  const int ycolA = (ka - p.kmin) * p.Cout + col, ycolB = (kb - p.kmin) * p.Cout + col;
  // the whole table as one buffer (ftmi_embed_bank checks it is below 2 GiB)
  const EbRsrc rs = __builtin_amdgcn_make_buffer_rsrc(
      (void *)p.tab, (short)0, (int)((unsigned)p.S * p.taps * p.Cout * 4u), 0x00020000);
  const unsigned voff = (unsigned)col * 4u;
  int t = r0 % p.T;
  int r = r0;
  if (p.pool && t > 0) {  // the row before the run, for the first row's pool
    --r;
    --t;
  }
  bool bad = false;
  for (; r < r1; ++r) {
    A.load(p, rs, voff, idv, wlo, r, t);
    Bg.load(p, rs, voff, idv, wlo, r, t);
    const bool pool_prev = p.pool && t > 0;
    const f32x4 oa = A.finish(pool_prev);
    const f32x4 ob = Bg.finish(pool_prev);
    if (p.split) bad |= A.nan() || Bg.nan();
    if (r >= r0) {
      bad |= eb_store(p, r, ycolA, oa);
      if (KB > 0) bad |= eb_store(p, r, ycolB, ob);
    }
    if (++t == p.T) t = 0;
  }
  if (bad && p.status) atomicOr(p.status, 1u);
}

#define EB_CASES(F)                                                                        \
  F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15) F(16)

// One kernel size alone: every bank but the 16-kernel one (a prenet with prenet_k != 16 goes
// kernel size by kernel size through here) and the single-size form (kmin = kmax: a
// SeriesPredictor's first conv, which no model path calls — measured, DESIGN.md §4 — and
// tests/test_gpu_embed_bank.py keeps checked).  No loop around the switch: the cases'
// constants stay inside them.
__device__ __forceinline__ void eb_single(const EbParams &p, int idv, int wlo, int r0, int r1,
                                          int k, int col) {
  switch (k) {
#define EB_ONE(K_) \
  case K_: eb_run<K_, 0>(p, idv, wlo, r0, r1, k, k, col); break;
    EB_CASES(EB_ONE)
#undef EB_ONE
    default: break;
  }
}

__global__ __launch_bounds__(EB_WAVES * 64, 4) void embed_bank_kernel(const EbParams p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slice = blockIdx.x % p.slices;
  const int tile = blockIdx.x / p.slices;
  const int r0 = (tile * EB_WAVES + wave) * EB_ROWS;
  if (r0 >= p.M) return;
  const int r1 = min(r0 + EB_ROWS, p.M);
  const int col = blockIdx.y * EB_PANEL + lane * 4;

  // ids of the rows the run's taps can touch: [r0 - 1 - kmax / 2, r1 + kmax - 1 - kmax / 2)
  const int wlo = r0 - 1 - EB_KMAX / 2;
  int idv = -1;
  {
    const int m = wlo + lane;
    if (m >= 0 && m < p.M) {
      const int64_t id = p.ids[m];
      if (id >= 0 && id < p.S) idv = (int)id;
    }
  }
  const int ka = p.kmin + slice, kb = p.kmax - slice;
  if (kb > ka && ka + kb == EB_KMAX + 1) {  // the 16-kernel bank's pairs: both in one pass
    switch (ka) {
#define EB_PAIR(K_) \
  case K_: eb_run<K_, EB_KMAX + 1 - K_>(p, idv, wlo, r0, r1, ka, kb, col); break;
      EB_PAIR(1) EB_PAIR(2) EB_PAIR(3) EB_PAIR(4) EB_PAIR(5) EB_PAIR(6) EB_PAIR(7) EB_PAIR(8)
#undef EB_PAIR
      default: break;
    }
    return;
  }
  eb_single(p, idv, wlo, r0, r1, ka, col);
  if (kb > ka) eb_single(p, idv, wlo, r0, r1, kb, col);
}

}  // namespace

extern "C" int ftmi_embed_bank(const int64_t *ids, int32_t B, int32_t T, const float *table,
                               int32_t num_rows, int32_t kmin, int32_t kmax, int32_t Cout,
                               const float *bn_scale, const float *bn_shift, float *y,
                               int64_t y_stride, int32_t flags, uint32_t *status,
                               ftmi_stream_t stream) {
  if (!ids || !table || !bn_scale || !bn_shift || !y || B <= 0 || T <= 0 || num_rows <= 0 ||
      Cout <= 0 || kmin < 1 || kmax < kmin)
    return FTMI_E_ARG;
  if (flags & ~(FTMI_BANK_POOL | FTMI_BANK_Y_SPLIT)) return FTMI_E_ARG;
  if (kmax > EB_KMAX || Cout % EB_PANEL) return FTMI_E_UNSUPPORTED;
  const int G = kmax - kmin + 1;
  const int64_t taps = (kmax * (kmax + 1) - kmin * (kmin - 1)) / 2;
  if ((int64_t)num_rows * taps * Cout * 4 >= ((int64_t)1 << 31)) return FTMI_E_UNSUPPORTED;
  if ((int64_t)B * T > INT32_MAX - 64 || y_stride < (int64_t)G * Cout) return FTMI_E_SHAPE;
  if (!ftmi_aligned16(table) || !ftmi_aligned16(bn_scale) || !ftmi_aligned16(bn_shift) ||
      !ftmi_aligned16(y) || (y_stride & 3))
    return FTMI_E_ALIGN;
  EbParams p = {};
  p.ids = ids;
  p.T = T;
  p.M = B * T;
  p.tab = table;
  p.S = num_rows;
  p.taps = (int)taps;
  p.Cout = Cout;
  p.kmin = kmin;
  p.kmax = kmax;
  p.slices = (G + 1) / 2;
  p.scale = bn_scale;
  p.shift = bn_shift;
  p.y = y;
  p.y_stride = y_stride;
  p.pool = (flags & FTMI_BANK_POOL) != 0;
  p.split = (flags & FTMI_BANK_Y_SPLIT) != 0;
  p.status = status;
  const int64_t tiles = ((int64_t)p.M + EB_WAVES * EB_ROWS - 1) / (EB_WAVES * EB_ROWS);
  if (tiles * p.slices > INT32_MAX) return FTMI_E_SHAPE;
  hipLaunchKernelGGL(embed_bank_kernel, dim3((unsigned)(tiles * p.slices), Cout / EB_PANEL),
                     dim3(EB_WAVES * 64), 0, ftmi_hs(stream), p);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}
