// The fused CBHG tail (ftmi_highway_stack, its few-row spread form) and the row-panel
// projection (ftmi_panel_proj*) on the f16x3 path.
#include "gemm.h"

using namespace ftmi_gemm;

namespace {

// ---- highway stack: pre_highway -> L highways -> GRU input projection, one launch -------
// models/common_layers.py:110-115 (CBHG: x = pre_highway(x); for h in highways: x = h(x);
// then the bidirectional GRU, whose input projection x W_ih^T + b_ih is the last GEMM here).
// The unfused chain writes and re-reads the (M, 256) activations in HBM between every layer
// and its short-K launches (K = 256: 8 k-steps per 256 x 128 tile) are prologue-bound.  Here
// one workgroup owns 64 rows x all 256 channels for the whole chain: 8 waves, wave w owns h
// columns [32w, 32w + 32).  Each layer's output is split (f16 head / scaled tail, as the
// other f16x3 kernels) into one of two LDS images — the next layer's A operand — while the
// wave keeps its own 64 x 32 block in fp32 registers: exactly the x its next gating needs,
// since the W1 and W2 columns of one h column (packed 32-column blocks) land in the same lane.
// B fragments (the pre-split f16 planes; every workgroup reads the same 1.4 MB, L2-resident)
// are loaded straight into registers three k-steps ahead; each GEMM runs in 16-column
// halves (a highway's W1 tile with its W2 tile) to keep that ring in the register budget.
// (A 128-row variant with 8 waves x 128 x 32 measured 671 vs 694 us at the c3 postnet and
// 209 vs 121 us at the prenet, where 100 tiles leave CUs idle: dropped.)  Per k-step, per product, the MFMA
// order and the epilogue arithmetic are the slab kernel's, so the result is bit-identical to
// the unfused chain.  HBM traffic per row: Cp floats in, n_out floats out (+ C with h).
constexpr int HS_BM = 64;
constexpr int HS_C = 256;
constexpr int HS_P = HS_C + 16;  // halves per LDS row: conflict-free ds_read_b128 fragments
constexpr int HS_IMG = HS_BM * HS_P;
constexpr int HS_MAXL = 8;
constexpr int HS_NPASS = 512;  // output-projection columns per pass (8 waves x 64)

struct HwStackParams {
  const float *x;
  int64_t x_stride;
  int M, Cp, kp_pre;      // rows, input channels, K of the pre_highway planes (roundup 32)
  const _Float16 *w_pre;  // f16 planes [3][C][kp_pre] (B0 = 2^11 w_h, B1 = w_t, B2 = w_h)
  const float *cs_pre;    // its column scales
  int L;
  const _Float16 *w_hw[HS_MAXL];  // [3][2C][C], W1 | W2 packed in 32-row blocks
  const float *cs_hw[HS_MAXL];
  const float *b1[HS_MAXL];
  const float *b2[HS_MAXL];
  const _Float16 *w_out;  // [3][n_out][C] (null: no projection)
  const float *cs_out;
  const float *b_out;
  int n_out;
  float *y;
  int64_t y_stride;
  float *h;  // optional: the last highway's output (fp32)
  int64_t h_stride;
  unsigned *status;
};

// acc[mi][ni] (rows 16 mi + 4 fs + i, GEMM column of bp[ni] + fr) = A x B^T over nks k-steps
// of 32, f16x3 (small terms first, as the slab kernel).  bp[ni]: the lane's B0 row + 8 fs.
template <int NI, int MI = 4>
__device__ __forceinline__ void hs_step(f32x4 (&acc)[MI][NI], const _Float16 *Ah,
                                        const _Float16 *At, const f16x8 (&b0)[NI],
                                        const f16x8 (&b1)[NI], int ks, int fr, int fs) {
  f16x8 bh[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) bh[ni] = b0[ni] * (_Float16)(1.0f / H3_SCALE);
  if constexpr (MI > 4) {  // the A fragments of row block mi + 1 read under the MFMAs of mi,
                           // one block ahead only (register budget: sched barriers)
    f16x8 ah = *(const f16x8 *)(Ah + fr * HS_P + 32 * ks + 8 * fs);
    f16x8 at = *(const f16x8 *)(At + fr * HS_P + 32 * ks + 8 * fs);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      f16x8 nh = ah, nt = at;
      if (mi + 1 < MI) {
        const int o = (16 * (mi + 1) + fr) * HS_P + 32 * ks + 8 * fs;
        nh = *(const f16x8 *)(Ah + o);
        nt = *(const f16x8 *)(At + o);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        f32x4 c = acc[mi][ni];
        c = mma16(at, bh[ni], c);
        c = mma16(ah, b1[ni], c);
        c = mma16(ah, b0[ni], c);
        acc[mi][ni] = c;
      }
      __builtin_amdgcn_sched_barrier(0);
      ah = nh;
      at = nt;
    }
    return;
  }
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {  // A fragments one row block at a time (register budget)
    const int o = (16 * mi + fr) * HS_P + 32 * ks + 8 * fs;
    const f16x8 ah = *(const f16x8 *)(Ah + o);
    const f16x8 at = *(const f16x8 *)(At + o);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      f32x4 c = acc[mi][ni];
      c = mma16(at, bh[ni], c);
      c = mma16(ah, b1[ni], c);
      c = mma16(ah, b0[ni], c);
      acc[mi][ni] = c;
    }
  }
}

// acc[mi][ni] (rows 16 mi + 4 fs + i, GEMM column of bp[ni] + fr) = A x B^T over nks k-steps
// of 32, f16x3 (small terms first, as the slab kernel).  bp[ni]: the lane's B0 row + 8 fs.
// B fragments rotate through three register sets, loaded three k-steps ahead (the loop is
// kept rolled and the steps fenced by sched barriers: otherwise the compiler hoists further
// loads and LDS reads across steps and spills).
template <int NI, int MI = 4>
__device__ __forceinline__ void hs_gemm_acc(f32x4 (&acc)[MI][NI], const _Float16 *Ah,
                                            const _Float16 *At, const _Float16 *const (&bp)[NI],
                                            int64_t plane, int nks, int fr, int fs) {
  // three register sets in a ring: the loads of k-step ks + 3 are issued right after step
  // ks consumed its set (one step of look-ahead left the L2 latency exposed: the MFMAs of a
  // step are ~800 cycles per wave, a loaded L2 round trip is more)
  f16x8 x0[NI], x1[NI], y0[NI], y1[NI], z0[NI], z1[NI];
  auto load = [&](f16x8 (&r0)[NI], f16x8 (&r1)[NI], int ks) {
    const int k = ks < nks ? ks : nks - 1;  // past the end: a clamped (unused) re-read
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      r0[ni] = *(const f16x8 *)(bp[ni] + 512 * k);
      r1[ni] = *(const f16x8 *)(bp[ni] + plane + 512 * k);
    }
  };
  load(x0, x1, 0);
  load(y0, y1, 1);
  load(z0, z1, 2);
#pragma unroll 1
  for (int ks = 0; ks < nks; ks += 3) {
    hs_step<NI, MI>(acc, Ah, At, x0, x1, ks, fr, fs);
    load(x0, x1, ks + 3);
    __builtin_amdgcn_sched_barrier(0);  // no hoisting across steps (register budget)
    if (ks + 1 >= nks) break;
    hs_step<NI, MI>(acc, Ah, At, y0, y1, ks + 1, fr, fs);
    load(y0, y1, ks + 4);
    __builtin_amdgcn_sched_barrier(0);
    if (ks + 2 >= nks) break;
    hs_step<NI, MI>(acc, Ah, At, z0, z1, ks + 2, fr, fs);
    load(z0, z1, ks + 5);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int NI, int MI = 4>
__device__ __forceinline__ void hs_gemm(f32x4 (&acc)[MI][NI], const _Float16 *Ah,
                                        const _Float16 *At, const _Float16 *const (&bp)[NI],
                                        int64_t plane, int nks, int fr, int fs) {
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
  hs_gemm_acc<NI, MI>(acc, Ah, At, bp, plane, nks, fr, fs);
}

// BM = 64: two LDS images, ping-pong (each layer reads one, writes the other); BM = 96: one
// image of 96 rows, overwritten in place behind a barrier (104 KB) — each weight fragment a
// wave fetches then feeds 6 row blocks instead of 4, cutting the per-CU L2 fetch per flop,
// which is what bounds this kernel, by a third.
template <int BM>
__global__ __launch_bounds__(512, 1) void highway_stack_kernel(const HwStackParams p) {
  constexpr int MI = BM / 16, NIMG = BM == 64 ? 2 : 1, IMG = BM * HS_P;
  static_assert(BM == 64 || BM == 96, "rows per workgroup");
  __shared__ __attribute__((aligned(16))) _Float16 lds[NIMG * 2 * IMG];  // [image][head|tail]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fs = lane >> 4;
  // column block of this wave, rotated per workgroup so that the CUs of one XCD (blocks
  // b, b + 8, ...) stream different weight rows at any moment instead of all hitting the
  // same L2 lines (channel hot spots); the arithmetic per column is unchanged
  const int cb = (wave + (blockIdx.x >> 3)) & 7;
  // the lane's B0 fragment of columns [n0, n0 + 16), k-step 0, in the fragment-major planes
  // [N/16][Kpad/32][64 lanes][8] (ftmi_split_weights_f16_frag): every wave load is one
  // contiguous 1-KB run (8 whole cache lines; row-major planes cost 16 half lines, measured
  // 1.48x slower at c3: the per-CU fetch rate, not MFMA, bounds this kernel)
  auto bptr = [&](const _Float16 *base, int n0, int Kpad) -> const _Float16 * {
    return base + (int64_t)(n0 >> 4) * (Kpad / 32) * 512 + lane * 8;
  };
  const int m0 = blockIdx.x * BM;
  float amax = 0.f;  // range guard: largest |activation| fed to the f16 split

  // ---- the input rows (Cp channels, zero-padded to kp_pre; rows past M zero) -> image 0
  const int q4 = p.kp_pre / 4;
  for (int e = tid; e < BM * q4; e += 512) {
    const int r = e / q4, c = (e - r * q4) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (m0 + r < p.M && c < p.Cp) v = *(const f32x4 *)(p.x + (int64_t)(m0 + r) * p.x_stride + c);
    amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    f16x4 hh, tt;
    split2h(v, hh, tt);
    *(f16x4 *)(lds + r * HS_P + c) = hh;
    *(f16x4 *)(lds + IMG + r * HS_P + c) = tt;
  }
  __syncthreads();

  f32x4 xs[MI][2];  // this wave's BM x 32 block of the current activations, fp32
  auto put = [&](int img) {  // xs -> LDS image img (split)
    _Float16 *Hd = lds + img * 2 * IMG, *Tl = Hd + IMG;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int nj = 0; nj < 2; ++nj)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = xs[mi][nj][i];
          amax = fmaxf(amax, fabsf(v));
          const _Float16 hh = (_Float16)v;
          const int o = (16 * mi + 4 * fs + i) * HS_P + 32 * cb + 16 * nj + fr;
          Hd[o] = hh;
          Tl[o] = (_Float16)((v - (float)hh) * H3_SCALE);
        }
  };

  // ---- pre_highway (Linear, no bias): x W_pre^T, K = kp_pre
  {
    f32x4 acc[MI][2];
    const _Float16 *bp[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
      bp[ni] = bptr(p.w_pre, 32 * cb + 16 * ni, p.kp_pre);
    hs_gemm<2, MI>(acc, lds, lds + IMG, bp, (int64_t)HS_C * p.kp_pre, p.kp_pre / 32, fr, fs);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const float cs = p.cs_pre[32 * cb + 16 * ni + fr];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) xs[mi][ni] = acc[mi][ni] * cs;
    }
  }
  int cur = NIMG - 1;
  if (NIMG == 1) __syncthreads();  // every wave is done reading the input image
  put(cur);
  __syncthreads();

  // ---- highways: g = sigmoid(x W2^T + b2), x <- g relu(x W1^T + b1) + (1 - g) x
  for (int l = 0; l < p.L; ++l) {
    const _Float16 *A = lds + cur * 2 * IMG;
    // two halves: W1 tile nj with its W2 tile (GEMM columns 64 cb + 16 nj, + 32), so one
    // half's accumulators and B ring stay small
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
      f32x4 acc[MI][2];
      const _Float16 *bp[2] = {bptr(p.w_hw[l], 64 * cb + 16 * nj, HS_C),
                               bptr(p.w_hw[l], 64 * cb + 32 + 16 * nj, HS_C)};
      hs_gemm<2, MI>(acc, A, A + IMG, bp, (int64_t)2 * HS_C * HS_C, HS_C / 32, fr, fs);
      const int col = 32 * cb + 16 * nj + fr;
      const float c1 = p.cs_hw[l][64 * cb + 16 * nj + fr];
      const float c2 = p.cs_hw[l][64 * cb + 32 + 16 * nj + fr];
      const float bb1 = p.b1[l][col], bb2 = p.b2[l][col];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float x1, x2;
          {
#pragma clang fp contract(off)
            // rounded like the slab kernel: the column scale, then the bias
            x1 = acc[mi][0][i] * c1 + bb1;
            x2 = acc[mi][1][i] * c2 + bb2;
          }
          const float g = ftmi_sigmoid(x2);
          xs[mi][nj][i] = highway_mix(g, x1, xs[mi][nj][i]);
        }
    }
    if (NIMG == 2) {
      cur ^= 1;  // the image read two layers ago: every wave passed the barrier since
    } else {
      __syncthreads();  // every wave is done reading the image it overwrites
    }
    put(cur);
    __syncthreads();
  }
  if (p.h) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = m0 + 16 * mi + 4 * fs + i;
        if (row >= p.M) continue;
#pragma unroll
        for (int nj = 0; nj < 2; ++nj)
          p.h[(int64_t)row * p.h_stride + 32 * cb + 16 * nj + fr] = xs[mi][nj][i];
      }
  }

  // ---- output projection (the GRU's x W_ih^T + b_ih), HS_NPASS columns per pass
  if (p.w_out) {
    const _Float16 *A = lds + cur * 2 * IMG;
    for (int q = 0; q < 2 * p.n_out / HS_NPASS; ++q) {  // 256 columns (32 per wave) a pass
      f32x4 acc[MI][2];
      const int n0 = (HS_NPASS / 2) * q + 32 * cb;
      const _Float16 *bp[2] = {bptr(p.w_out, n0, HS_C), bptr(p.w_out, n0 + 16, HS_C)};
      hs_gemm<2, MI>(acc, A, A + IMG, bp, (int64_t)p.n_out * HS_C, HS_C / 32, fr, fs);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int col = n0 + 16 * ni + fr;
        const float cs = p.cs_out[col], b = p.b_out ? p.b_out[col] : 0.f;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)
            const int row = m0 + 16 * mi + 4 * fs + i;
            float v = acc[mi][ni][i] * cs;
            if (p.b_out) v += b;
            if (row < p.M) p.y[(int64_t)row * p.y_stride + col] = v;
          }
      }
    }
  }
  if (!(amax <= 65504.f) && p.status) atomicOr(p.status, 1u);
}

// ---- the CBHG tail for few rows, spread over the chip (c2: 120 / 816 rows) -------------
// highway_stack_kernel gives one workgroup 64 rows x ALL 256 channels, so at batch 1 (120
// prenet rows: 2 workgroups; 816 postnet rows: 13) a few CUs stream the whole 3-4 MB of
// weight planes each (~100 us).  Here a row block is spread over HSS_P = 16 workgroups, each
// owning 16 output channels of every layer (and n_out / 16 columns of the output
// projection): it streams 1/16 of the weights, and the layers' activations are exchanged
// between the 16 workgroups of a row block through memory after each layer.  Exchange
// (MI355X_MICROARCH.md "Valid forms", first row of the sc1 table): a workgroup writes its
// 64 x 16 slice of the layer's output, split into the f16 head / scaled-tail image layout,
// with 16-B sc1 stores; every storing wave waits for its stores (vmcnt(0)); a barrier; one
// lane adds to the row block's counter (agent scope) and polls it (sc1 loads, bounded) until
// all 16 have added for this layer; a barrier; then every wave loads the full 64 x 256 image
// with sc1 loads into LDS.  The image buffers alternate by layer parity: a workgroup writes
// layer l + 2's slice only after all 16 have published layer l + 1, which each did after
// reading layer l's image.  Per accumulator the k-step, product and epilogue order of
// highway_stack_kernel (hs_gemm over the same fragment-major planes, one 16-row block per
// wave): the results are bit-identical to it.  Every workgroup must be resident at once
// (RB x 16 <= the CU count: the host checks); a spin past the bound sets the status word's
// timeout bit (FTMI_STATUS_RNN_TIMEOUT) instead of hanging.
constexpr int HSS_P = 16;       // workgroups (channel slices) per row block
constexpr int HSS_MAXRB = 16;   // row blocks: M <= 1024
constexpr int HSS_CNT = 32;     // words between row-block counters (one 128-B line each)

struct HsSpread {
  unsigned *cnt;    // [RB][HSS_CNT] arrival counters, zeroed before the launch
  _Float16 *xb;     // [2][RB][2 planes][HS_BM][HS_P] exchange images
  unsigned spin;    // poll bound
};

template <int NO>
__global__ __launch_bounds__(512, 1) void highway_spread_kernel(const HwStackParams p,
                                                               const HsSpread q) {
  constexpr int IMG = HS_IMG;
  __shared__ __attribute__((aligned(16))) _Float16 lds[2 * IMG];           // head | tail
  __shared__ __attribute__((aligned(16))) _Float16 pub[2 * HS_BM * 16];   // the slice, split
  __shared__ int s_abort;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fs = lane >> 4;
  const int s = blockIdx.x % HSS_P, rb = blockIdx.x / HSS_P;
  const int m0 = rb * HS_BM, mi = wave & 3;
  const int RB = (p.M + HS_BM - 1) / HS_BM;
  auto bptr = [&](const _Float16 *base, int n0, int Kpad) -> const _Float16 * {
    return base + (int64_t)(n0 >> 4) * (Kpad / 32) * 512 + lane * 8;
  };
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(q.xb, (short)0, 0x7FFFFFF0, 0x00020000);
  const int img_halves = 2 * HS_BM * HS_P;  // one (parity, row block) image
  float amax = 0.f;
  if (tid == 0) s_abort = 0;

  // ---- the input rows -> the LDS image (as highway_stack_kernel)
  const int q4 = p.kp_pre / 4;
  for (int e = tid; e < HS_BM * q4; e += 512) {
    const int r = e / q4, c = (e - r * q4) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (m0 + r < p.M && c < p.Cp) v = *(const f32x4 *)(p.x + (int64_t)(m0 + r) * p.x_stride + c);
    amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    f16x4 hh, tt;
    split2h(v, hh, tt);
    *(f16x4 *)(lds + r * HS_P + c) = hh;
    *(f16x4 *)(lds + IMG + r * HS_P + c) = tt;
  }
  __syncthreads();
  const _Float16 *Ah = lds + 16 * mi * HS_P, *At = lds + IMG + 16 * mi * HS_P;

  // waves 0-3: rows 16 mi + 4 fs + i, channel 16 s + fr of the current activations (fp32)
  f32x4 xs = {0.f, 0.f, 0.f, 0.f};
  if (wave < 4) {  // pre_highway (no bias)
    f32x4 acc[1][1];
    const _Float16 *bp[1] = {bptr(p.w_pre, 16 * s, p.kp_pre)};
    hs_gemm<1, 1>(acc, Ah, At, bp, (int64_t)HS_C * p.kp_pre, p.kp_pre / 32, fr, fs);
    xs = acc[0][0] * p.cs_pre[16 * s + fr];
  }

  // publish xs as layer l's slice, wait for the row block's 16 slices, load the image
  auto exchange = [&](int l) -> bool {
    if (wave < 4) {  // the slice, split, into pub [plane][row][16]
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = xs[i];
        amax = fmaxf(amax, fabsf(v));
        const _Float16 hh = (_Float16)v;
        const int o = (16 * mi + 4 * fs + i) * 16 + fr;
        pub[o] = hh;
        pub[HS_BM * 16 + o] = (_Float16)((v - (float)hh) * H3_SCALE);
      }
    }
    __syncthreads();
    const int par = l & 1;
    const int base = (par * RB + rb) * img_halves;  // halves
    if (tid < 256) {  // 16-B chunk (plane, row, half of the 16 channels), write-through
      const int pl = tid >> 7, row = (tid >> 1) & 63, c8 = tid & 1;
      const u32x4 v = *(const u32x4 *)(pub + (pl * HS_BM + row) * 16 + 8 * c8);
      const int off = (base + (pl * HS_BM + row) * HS_P + 16 * s + 8 * c8) * 2;
      __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, 16 /* sc1 */);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave's stores done
    __syncthreads();
    if (tid == 0) {
      unsigned *c = q.cnt + rb * HSS_CNT;
      __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned want = (unsigned)HSS_P * (l + 1);
      unsigned spins = 0;
      while (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > q.spin) {
          s_abort = 1;
          if (p.status) atomicOr(p.status, FTMI_STATUS_RNN_TIMEOUT);
          break;
        }
      }
    }
    __syncthreads();
    if (s_abort) return false;
    u32x4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // chunk e = (plane, row, 16-B piece of the 256 channels)
      const int e = tid + 512 * j, pl = e >> 11, row = (e >> 5) & 63, c = e & 31;
      v[j] = __builtin_amdgcn_raw_buffer_load_b128(
          rs, (base + (pl * HS_BM + row) * HS_P + 8 * c) * 2, 0, 16 /* sc1 */);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = tid + 512 * j, pl = e >> 11, row = (e >> 5) & 63, c = e & 31;
      *(u32x4 *)(lds + pl * IMG + row * HS_P + 8 * c) = v[j];
    }
    __syncthreads();
    return true;
  };

  // ---- highways: g = sigmoid(x W2^T + b2), x <- g relu(x W1^T + b1) + (1 - g) x
  for (int l = 0; l < p.L; ++l) {
    if (!exchange(l)) return;
    if (wave < 4) {
      const int cb = s >> 1, nj = s & 1;  // the stack kernel's (column block, half)
      f32x4 acc[1][2];
      const _Float16 *bp[2] = {bptr(p.w_hw[l], 64 * cb + 16 * nj, HS_C),
                               bptr(p.w_hw[l], 64 * cb + 32 + 16 * nj, HS_C)};
      hs_gemm<2, 1>(acc, Ah, At, bp, (int64_t)2 * HS_C * HS_C, HS_C / 32, fr, fs);
      const int col = 16 * s + fr;
      const float c1 = p.cs_hw[l][64 * cb + 16 * nj + fr];
      const float c2 = p.cs_hw[l][64 * cb + 32 + 16 * nj + fr];
      const float bb1 = p.b1[l][col], bb2 = p.b2[l][col];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float x1, x2;
        {
#pragma clang fp contract(off)
          x1 = acc[0][0][i] * c1 + bb1;
          x2 = acc[0][1][i] * c2 + bb2;
        }
        const float g = ftmi_sigmoid(x2);
        xs[i] = highway_mix(g, x1, xs[i]);
      }
    }
  }
  if (p.h && wave < 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = m0 + 16 * mi + 4 * fs + i;
      if (row < p.M) p.h[(int64_t)row * p.h_stride + 16 * s + fr] = xs[i];
    }
  }

  // ---- output projection: columns [n_out / 16 s, + n_out / 16), two halves of NO tiles
  if (p.w_out) {
    if (!exchange(p.L)) return;
    const int n0 = (p.n_out / HSS_P) * s + (wave >> 2) * 16 * NO;
    f32x4 acc[1][NO];
    const _Float16 *bp[NO];
#pragma unroll
    for (int ni = 0; ni < NO; ++ni) bp[ni] = bptr(p.w_out, n0 + 16 * ni, HS_C);
    hs_gemm<NO, 1>(acc, Ah, At, bp, (int64_t)p.n_out * HS_C, HS_C / 32, fr, fs);
#pragma unroll
    for (int ni = 0; ni < NO; ++ni) {
      const int col = n0 + 16 * ni + fr;
      const float cs = p.cs_out[col], b = p.b_out ? p.b_out[col] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)
        const int row = m0 + 16 * mi + 4 * fs + i;
        float v = acc[0][ni][i] * cs;
        if (p.b_out) v += b;
        if (row < p.M) p.y[(int64_t)row * p.y_stride + col] = v;
      }
    }
  }
  if (!(amax <= 65504.f) && p.status) atomicOr(p.status, 1u);
}

// ---- row-panel projection: y = [LayerNorm](x W^T + b [+ residual]) --------------------
// The k = 1 contractions of a FastPitch FFT block (models/fast_pitch.py:56-91, the
// reference's FFTBlock): self_attn.in_proj (K = d, N = 3d), out_proj + residual -> norm1
// (K = N = d) and conv2 (k = 1) + residual -> norm2 (K = d_fft, N = d).  At d = 256 these are
// short-K or narrow-N GEMMs: the 256 x 128 slab tiles run them at 90-170 TF/s, prologue and
// epilogue bound, and each LayerNorm is one more read + write of the rows.  Here a workgroup
// owns 64 rows: their channels are staged once per 256-channel chunk into an f16 head /
// scaled tail LDS image (the highway stack's layout and k-step code, hs_gemm_acc), the 8
// waves sweep 256-column panels (wave = 32 columns, B fragments from the L2-resident
// fragment-major planes), and the epilogue applies colscale and bias into an LDS row tile,
// then adds the residual and — for a 256-column output — runs the LayerNorm one wave per
// row with layernorm_kernel<4>'s arithmetic, writing each row once with coalesced stores.
// Per k-step, product and epilogue rounding the slab kernel's order: the projection
// values are bit-identical to conv1d's.  HBM per row: K floats in, N out (+ N residual).
constexpr int PP_BM = 64;
constexpr int PP_KC = HS_C;    // channels per staged chunk
constexpr int PP_TP = HS_C + 4;  // floats per LDS tile row (conflict-free fragment stores)

struct PanelParams {
  const float *x;
  int64_t x_stride;
  int M, K, kpad, N;
  const _Float16 *w;  // split_weights_f16_frag planes [3][N/16][kpad/32][64][8]
  const float *cs;    // their column scales
  const float *bias;
  const float *res;
  int64_t res_stride;
  const float *ln_g, *ln_b;  // LayerNorm over the N = 256 columns (null: none)
  float eps;
  float *y;
  int64_t y_stride;
  unsigned *status;
  // ftmi_panel_proj_qkv: panels 1 and 2 (K, V of the in_proj output) go to the attention
  // workspace as f16 head / scaled tail planes instead of y (ftmi_attention's layout: K
  // [B*H][Tp][hd], V transposed [B*H][hd][Tp]); rows are (b, key) = (row / T, row % T)
  _Float16 *kv;
  int T, H, hd, Tp;
};

// Persistent over row tiles (grid = min(tiles, CUs)): the next job's channels (the next
// chunk, or the next tile's first) are loaded into registers right after the current chunk
// is staged, so their HBM latency hides behind this chunk's MFMAs (the residual rows of a
// panel are issued at once ahead of its tile writes); one workgroup per CU (136 KB LDS).
__global__ __launch_bounds__(512) void panel_proj_kernel(const PanelParams p) {
  __shared__ __attribute__((aligned(16))) _Float16 lds[2 * HS_IMG];   // head | tail
  __shared__ __attribute__((aligned(16))) float tile[PP_BM * PP_TP];  // finished panel rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fs = lane >> 4;
  // column block of this wave, rotated per workgroup (highway_stack_kernel: spreads the
  // concurrent B reads of one XCD over different weight lines)
  const int cb = (wave + (blockIdx.x >> 3)) & 7;
  const int ntiles = (p.M + PP_BM - 1) / PP_BM;
  const int nch = (p.kpad + PP_KC - 1) / PP_KC, nq = p.N / HS_C;
  const bool ln = p.ln_g != nullptr;
  float amax = 0.f;
  f32x4 ra[8];  // one job's channels: rows wave + 8 u, channels c0 + 4 lane .. + 3
  auto load_job = [&](int t, int c) {
    const int c0 = c * PP_KC, kc = min(PP_KC, p.kpad - c0);
    const float *xb = p.x + (int64_t)(t * PP_BM + wave) * p.x_stride + c0 + 4 * lane;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      ra[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (4 * lane < kc && t * PP_BM + wave + 8 * u < p.M && c0 + 4 * lane < p.K)
        ra[u] = *(const f32x4 *)(xb + (int64_t)8 * u * p.x_stride);
    }
  };
  auto store_job = [&](int c) {  // ra -> the LDS image (f16 head / scaled tail)
    if (4 * lane >= min(PP_KC, p.kpad - c * PP_KC)) return;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const f32x4 v = ra[u];
      amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
      f16x4 hh, tt;
      split2h(v, hh, tt);
      const int o = (wave + 8 * u) * HS_P + 4 * lane;
      *(f16x4 *)(lds + o) = hh;
      *(f16x4 *)(lds + HS_IMG + o) = tt;
    }
  };
  // the residual of panel q, in the row pass's layout: LN — wave w rows 8w + u, columns
  // lane + 64 j (rv[u][j]); plain — rows w + 8u, columns 4 lane .. + 3 (rv[u] as a float4)
  float rv[8][4];
  auto load_res = [&](int t, int q) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int row = t * PP_BM + (ln ? 8 * wave + u : wave + 8 * u);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (p.res && row < p.M) {
        const float *rr = p.res + (int64_t)row * p.res_stride + HS_C * q;
        if (ln) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = rr[lane + 64 * j];
        } else {
          v = *(const f32x4 *)(rr + 4 * lane);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) rv[u][j] = v[j];
    }
  };

  int t = blockIdx.x;
  if (t >= ntiles) return;
  load_job(t, 0);
#pragma unroll 1
  for (;; ) {
#pragma unroll 1
    for (int q = 0; q < nq; ++q) {
      f32x4 acc[4][2];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
      for (int c = 0; c < nch; ++c) {
        if (nch > 1 || q == 0) {  // one chunk: staged once for every panel
          __syncthreads();        // every wave is past its reads of the image
          store_job(c);
          __syncthreads();
          // the next job's channels, in flight during this chunk's MFMAs
          if (c + 1 < nch)
            load_job(t, c + 1);
          else if (nch > 1 && q + 1 < nq)
            load_job(t, 0);
          else if (t + (int)gridDim.x < ntiles)
            load_job(t + gridDim.x, 0);
        }
        const _Float16 *bp[2];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          bp[ni] = p.w + (int64_t)((HS_C * q + 32 * cb + 16 * ni) >> 4) * (p.kpad / 32) * 512 +
                   lane * 8 + 512 * (PP_KC / 32) * c;
        hs_gemm_acc<2>(acc, lds, lds + HS_IMG, bp, (int64_t)p.N * p.kpad,
                       min(PP_KC, p.kpad - c * PP_KC) / 32, fr, fs);
      }
      // ---- epilogue, the slab kernel's rounding order: t = acc colscale (+ bias) into the
      // LDS row tile, then row passes: (+ residual), [LayerNorm], coalesced stores
      load_res(t, q);  // in flight during the tile writes and the barrier
      if (q > 0) __syncthreads();  // the previous panel's row pass is done with the tile
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int col = HS_C * q + 32 * cb + 16 * ni + fr;
        const float cs = p.cs[col], b = p.bias ? p.bias[col] : 0.f;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)
            float v = acc[mi][ni][i] * cs;
            if (p.bias) v += b;
            tile[(16 * mi + 4 * fs + i) * PP_TP + 32 * cb + 16 * ni + fr] = v;
          }
      }
      __syncthreads();
      const int m0 = t * PP_BM;
      if (p.kv && q >= 1) {  // K / V panel -> split planes (the attention split pass's values)
        const int64_t plane = (int64_t)(p.M / p.T) * p.H * p.Tp * p.hd;
        float amax = 0.f;
        if (q == 1) {  // K rows: lane = 4 consecutive columns of one head
          const int c = 4 * lane, hh = c / p.hd, d = c - hh * p.hd;
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int r = wave + 8 * u, row = m0 + r;
            if (row >= p.M) continue;
            const int b = row / p.T, key = row - b * p.T;
            const f32x4 v = *(const f32x4 *)(tile + r * PP_TP + c);
            amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
            f16x4 h4, t4;
            split2h(v, h4, t4);
            const int64_t o = ((int64_t)(b * p.H + hh) * p.Tp + key) * p.hd + d;
            *(f16x4 *)(p.kv + o) = h4;
            *(f16x4 *)(p.kv + plane + o) = t4;
          }
        } else {  // V^T: a thread takes 4 consecutive keys (rows) of one column, 8 B per plane
          // where they are 4 aligned keys of one sequence; a wave-instruction covers 16
          // columns x 4 row quads (conflict-free LDS reads at the 260-float pitch)
          for (int e = tid; e < HS_C * (PP_BM / 4); e += 512) {
            const int l = e & 63, wv = e >> 6;
            const int c = (wv & 15) * 16 + (l & 15), r0 = ((wv >> 4) * 4 + (l >> 4)) * 4;
            const int hh = c / p.hd, d = c - hh * p.hd;
            const int row0 = m0 + r0, b0 = row0 / p.T, key0 = row0 - b0 * p.T;
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = tile[(r0 + i) * PP_TP + c];
            if (row0 + 3 < p.M && key0 + 3 < p.T && (key0 & 3) == 0) {
              amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
              f16x4 h4, t4;
              split2h(v, h4, t4);
              const int64_t o = 2 * plane + ((int64_t)(b0 * p.H + hh) * p.hd + d) * p.Tp + key0;
              *(f16x4 *)(p.kv + o) = h4;
              *(f16x4 *)(p.kv + o + plane) = t4;
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int row = row0 + i;
                if (row >= p.M) break;
                const int b = row / p.T, key = row - b * p.T;
                amax = fmaxf(amax, fabsf(v[i]));
                const _Float16 h1 = (_Float16)v[i];
                const int64_t o = 2 * plane + ((int64_t)(b * p.H + hh) * p.hd + d) * p.Tp + key;
                p.kv[o] = h1;
                p.kv[o + plane] = (_Float16)((v[i] - (float)h1) * H3_SCALE);
              }
            }
          }
        }
        if (!(amax <= 65504.f) && p.status) atomicOr(p.status, 1u);
      } else if (!ln) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int r = wave + 8 * u, row = m0 + r;
          if (row >= p.M) continue;
          f32x4 v = *(const f32x4 *)(tile + r * PP_TP + 4 * lane);
          if (p.res) v += (f32x4){rv[u][0], rv[u][1], rv[u][2], rv[u][3]};
          *(f32x4 *)(p.y + (int64_t)row * p.y_stride + HS_C * q + 4 * lane) = v;
        }
      } else {  // one wave per row: layernorm_kernel<4>'s arithmetic (fp64 sums, same order)
        float gm[4], bt[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          gm[j] = p.ln_g[lane + 64 * j];
          bt[j] = p.ln_b[lane + 64 * j];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int r = 8 * wave + u, row = m0 + r;
          if (row >= p.M) break;
          float v[4];
          double sm = 0.0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[j] = tile[r * PP_TP + lane + 64 * j];
            if (p.res) v[j] += rv[u][j];
            sm += v[j];
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o);
          const double mean = sm / HS_C;
          double sq = 0.0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double d = (double)v[j] - mean;
            sq += d * d;
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
          const float rstd = (float)(1.0 / sqrt(sq / HS_C + (double)p.eps));
          const float meanf = (float)mean;
          const float nb = -(rstd * meanf);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
#pragma clang fp contract(off)
            p.y[(int64_t)row * p.y_stride + lane + 64 * j] = (v[j] * rstd + nb) * gm[j] + bt[j];
          }
        }
      }
    }
    t += gridDim.x;
    if (t >= ntiles) break;
  }
  if (!(amax <= 65504.f) && p.status) atomicOr(p.status, 1u);
}

// the current device's CU count as the runtime reports it (256 when the query fails)
static int device_cus() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 256;
  return n;
}

// f16 planes + column scales of a split_weights_f16 block [3][N][Kpad] + colscale[N]
static const float *f16_colscale(const void *w3, int64_t N, int64_t K) {
  const int64_t Kpad = (K + X6_BK - 1) / X6_BK * X6_BK;
  return (const float *)((const char *)w3 + 3 * N * Kpad * 2);
}

// the parameters of ftmi_highway_stack[_spread] (FTMI_OK or the argument error)
static int hs_params(HwStackParams &p, const float *x, int64_t x_stride, int64_t M, int32_t Cp,
                     int32_t C, const void *w_pre_split, int32_t L,
                     const void *const *w_hw_split, const float *const *b1,
                     const float *const *b2, const void *w_out_split, const float *b_out,
                     int32_t n_out, float *y, int64_t y_stride, float *h, int64_t h_stride,
                     uint32_t *status) {
  if (!x || !w_pre_split || M <= 0 || Cp <= 0 || L < 0) return FTMI_E_ARG;
  if (L > 0 && (!w_hw_split || !b1 || !b2)) return FTMI_E_ARG;
  if (w_out_split ? (!y || n_out <= 0) : (n_out != 0 || y != nullptr)) return FTMI_E_ARG;
  if (!y && !h) return FTMI_E_ARG;
  if (C != HS_C || Cp > HS_C || Cp % 4 != 0 || L > HS_MAXL) return FTMI_E_SHAPE;
  if (n_out % HS_NPASS != 0 || M > INT32_MAX) return FTMI_E_SHAPE;
  if (!ftmi_aligned16(x) || (x_stride & 3) || !ftmi_aligned16(w_pre_split)) return FTMI_E_ALIGN;
  if (w_out_split && !ftmi_aligned16(w_out_split)) return FTMI_E_ALIGN;
  if ((const float *)x == y || (const float *)x == h) return FTMI_E_ARG;
  p = HwStackParams{};
  p.x = x;
  p.x_stride = x_stride;
  p.M = (int)M;
  p.Cp = Cp;
  p.kp_pre = (Cp + X6_BK - 1) / X6_BK * X6_BK;
  p.w_pre = (const _Float16 *)w_pre_split;
  p.cs_pre = f16_colscale(w_pre_split, C, Cp);
  p.L = L;
  for (int l = 0; l < L; ++l) {
    if (!w_hw_split[l] || !b1[l] || !b2[l] || !ftmi_aligned16(w_hw_split[l])) return FTMI_E_ARG;
    p.w_hw[l] = (const _Float16 *)w_hw_split[l];
    p.cs_hw[l] = f16_colscale(w_hw_split[l], 2 * C, C);
    p.b1[l] = b1[l];
    p.b2[l] = b2[l];
  }
  if (w_out_split) {
    p.w_out = (const _Float16 *)w_out_split;
    p.cs_out = f16_colscale(w_out_split, n_out, C);
    p.b_out = b_out;
    p.n_out = n_out;
    p.y = y;
    p.y_stride = y_stride;
  }
  p.h = h;
  p.h_stride = h_stride;
  p.status = status;
  return FTMI_OK;
}

}  // namespace

extern "C" int ftmi_highway_stack(const float *x, int64_t x_stride, int64_t M, int32_t Cp,
                                  int32_t C, const void *w_pre_split, int32_t L,
                                  const void *const *w_hw_split, const float *const *b1,
                                  const float *const *b2, const void *w_out_split,
                                  const float *b_out, int32_t n_out, float *y, int64_t y_stride,
                                  float *h, int64_t h_stride, uint32_t *status,
                                  ftmi_stream_t stream) {
  HwStackParams p;
  const int rc = hs_params(p, x, x_stride, M, Cp, C, w_pre_split, L, w_hw_split, b1, b2,
                           w_out_split, b_out, n_out, y, y_stride, h, h_stride, status);
  if (rc != FTMI_OK) return rc;
  // 96 rows per workgroup once the grid still fills the chip (FTMI_HS_BM = 64 / 96, read per
  // call, forces one; 128 rows would need ~290 VGPRs and spills)
  const char *e = getenv("FTMI_HS_BM");
  const int bm = e ? atoi(e) : (M >= 96 * 256 ? 96 : 64);
  if (bm == 96) {
    const unsigned blocks = (unsigned)((M + 95) / 96);
    hipLaunchKernelGGL(highway_stack_kernel<96>, dim3(blocks), dim3(512), 0, ftmi_hs(stream), p);
  } else {
    const unsigned blocks = (unsigned)((M + HS_BM - 1) / HS_BM);
    hipLaunchKernelGGL(highway_stack_kernel<64>, dim3(blocks), dim3(512), 0, ftmi_hs(stream), p);
  }
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int64_t ftmi_highway_stack_spread_ws_bytes(int64_t M) {
  if (M <= 0 || M > (int64_t)HSS_MAXRB * HS_BM) return 0;
  const int64_t RB = (M + HS_BM - 1) / HS_BM;
  return RB * HSS_CNT * 4 + 2 * RB * 2 * HS_BM * HS_P * 2;
}

extern "C" int32_t ftmi_highway_stack_spread_blocks(int64_t M) {
  if (M <= 0 || M > (int64_t)HSS_MAXRB * HS_BM) return 0;
  return (int32_t)((M + HS_BM - 1) / HS_BM * HSS_P);
}

extern "C" int ftmi_highway_stack_spread(const float *x, int64_t x_stride, int64_t M, int32_t Cp,
                                         int32_t C, const void *w_pre_split, int32_t L,
                                         const void *const *w_hw_split, const float *const *b1,
                                         const float *const *b2, const void *w_out_split,
                                         const float *b_out, int32_t n_out, float *y,
                                         int64_t y_stride, float *h, int64_t h_stride,
                                         uint32_t *status, void *ws, ftmi_stream_t stream) {
  HwStackParams p;
  const int rc = hs_params(p, x, x_stride, M, Cp, C, w_pre_split, L, w_hw_split, b1, b2,
                           w_out_split, b_out, n_out, y, y_stride, h, h_stride, status);
  if (rc != FTMI_OK) return rc;
  if (!ws) return FTMI_E_ARG;
  if (!ftmi_aligned16(ws)) return FTMI_E_ALIGN;
  const int blocks = ftmi_highway_stack_spread_blocks(M);
  const int cus = device_cus();  // asked on every call
  // every workgroup resident at once (they wait on each other); n_out split in two halves
  // of n_out / 512 16-column tiles per slice
  if (blocks <= 0 || blocks > cus || (w_out_split && n_out > 3 * HS_NPASS)) return FTMI_E_UNSUPPORTED;
  {
    const int nk = w_out_split ? n_out / HS_NPASS : 1;
    const void *k = nk == 1 ? (const void *)highway_spread_kernel<1>
                  : nk == 2 ? (const void *)highway_spread_kernel<2>
                            : (const void *)highway_spread_kernel<3>;
    if (int rc2 = ftmi_resident_ok(k, blocks, 512, 0)) return rc2;
  }
  const int RB = blocks / HSS_P;
  HsSpread q;
  q.cnt = (unsigned *)ws;
  q.xb = (_Float16 *)((char *)ws + (int64_t)RB * HSS_CNT * 4);
  q.spin = 1u << 22;
  hipStream_t s = ftmi_hs(stream);
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)RB * HSS_CNT * 4, s);
  if (e != hipSuccess) return (int)e;
  switch (w_out_split ? n_out / HS_NPASS : 1) {
    case 1: hipLaunchKernelGGL(highway_spread_kernel<1>, dim3(blocks), dim3(512), 0, s, p, q); break;
    case 2: hipLaunchKernelGGL(highway_spread_kernel<2>, dim3(blocks), dim3(512), 0, s, p, q); break;
    default: hipLaunchKernelGGL(highway_spread_kernel<3>, dim3(blocks), dim3(512), 0, s, p, q);
  }
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

namespace {
static int panel_launch(PanelParams &p, int64_t M, hipStream_t stream) {
  static const int cus = [] {  // once per process
    const int n = device_cus();
    return n > 0 ? n : 256;
  }();
  const int64_t tiles = (M + PP_BM - 1) / PP_BM;
  const unsigned blocks = (unsigned)(tiles < cus ? tiles : cus);
  hipLaunchKernelGGL(panel_proj_kernel, dim3(blocks), dim3(512), 0, stream, p);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}
}  // namespace

extern "C" int ftmi_panel_proj_qkv(const float *x, int64_t x_stride, int32_t B, int32_t T,
                                   int32_t K, const void *w_split_frag, int32_t d,
                                   const float *bias, int32_t heads, float *q_out,
                                   int64_t q_stride, void *kv_workspace, int64_t workspace_bytes,
                                   uint32_t *status, ftmi_stream_t stream) {
  if (!x || !w_split_frag || !q_out || !kv_workspace || B <= 0 || T <= 0 || K <= 0) return FTMI_E_ARG;
  if (d != HS_C || heads <= 0 || d % heads) return FTMI_E_SHAPE;
  const int hd = d / heads;
  if (hd != 64 && hd != 128) return FTMI_E_UNSUPPORTED;
  const int64_t M = (int64_t)B * T;
  if (K % 4 || M > INT32_MAX || x_stride < K || q_stride < d) return FTMI_E_SHAPE;
  if (workspace_bytes < ftmi_attention_workspace_bytes(B, T, heads, hd)) return FTMI_E_SHAPE;
  if (!ftmi_aligned16(x) || (x_stride & 3) || !ftmi_aligned16(w_split_frag) ||
      !ftmi_aligned16(q_out) || (q_stride & 3) || !ftmi_aligned16(kv_workspace))
    return FTMI_E_ALIGN;
  if ((const float *)x == q_out) return FTMI_E_ARG;
  PanelParams p = {};
  p.x = x;
  p.x_stride = x_stride;
  p.M = (int)M;
  p.K = K;
  p.kpad = (K + X6_BK - 1) / X6_BK * X6_BK;
  p.N = 3 * d;
  p.w = (const _Float16 *)w_split_frag;
  p.cs = f16_colscale(w_split_frag, 3 * d, K);
  p.bias = bias;
  p.y = q_out;
  p.y_stride = q_stride;
  p.status = status;
  p.kv = (_Float16 *)kv_workspace;
  p.T = T;
  p.H = heads;
  p.hd = hd;
  p.Tp = (T + 63) / 64 * 64;
  return panel_launch(p, M, ftmi_hs(stream));
}

extern "C" int ftmi_panel_proj(const float *x, int64_t x_stride, int64_t M, int32_t K,
                               const void *w_split_frag, int32_t N, const float *bias,
                               const float *residual, int64_t res_stride, const float *ln_gamma,
                               const float *ln_beta, float eps, float *y, int64_t y_stride,
                               uint32_t *status, ftmi_stream_t stream) {
  if (!x || !w_split_frag || !y || M < 0 || K <= 0 || N <= 0) return FTMI_E_ARG;
  if (!ln_gamma != !ln_beta) return FTMI_E_ARG;
  if (K % 4 || N % HS_C || (ln_gamma && N != HS_C) || M > INT32_MAX) return FTMI_E_SHAPE;
  if (x_stride < K || y_stride < N || (residual && res_stride < N)) return FTMI_E_SHAPE;
  if (!ftmi_aligned16(x) || (x_stride & 3) || !ftmi_aligned16(w_split_frag)) return FTMI_E_ALIGN;
  // the rows of x are re-read after other workgroups' rows of y are written (chunks,
  // panels): no aliasing; y may alias the residual (each element read before its write)
  if ((const float *)x == y) return FTMI_E_ARG;
  if (M == 0) return FTMI_OK;
  PanelParams p = {};
  p.x = x;
  p.x_stride = x_stride;
  p.M = (int)M;
  p.K = K;
  p.kpad = (K + X6_BK - 1) / X6_BK * X6_BK;
  p.N = N;
  p.w = (const _Float16 *)w_split_frag;
  p.cs = f16_colscale(w_split_frag, N, K);
  p.bias = bias;
  p.res = residual;
  p.res_stride = res_stride;
  p.ln_g = ln_gamma;
  p.ln_b = ln_beta;
  p.eps = eps;
  p.y = y;
  p.y_stride = y_stride;
  p.status = status;
  return panel_launch(p, M, ftmi_hs(stream));
}
