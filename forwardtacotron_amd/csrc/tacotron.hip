// Tacotron decoder loop (reference: models/tacotron.py Decoder.forward :124-174 inside the
// loops of Tacotron.forward :250-256 and Tacotron.generate :304-312) on gfx950, as ONE
// persistent launch: no per-step launches, no per-step host syncs.
//
// Per decoder step s (frame t = s r) and batch item b the reference computes
//   p  = prenet(last frame)                       (free-running: the step's own output)
//   hA = GRUCell([ctx, p], hA)
//   u  = v . tanh(W hA + b + enc_proj + L conv([cum, att]) + b);  att = softmax_T(u)
//   cum += att;  ctx = att @ enc
//   x  = rnn_input([ctx, hA]);  (h1, c1) = LSTM1(x);  x += h1;  (h2, c2) = LSTM2(x);  x += h2
//   frames = mel_proj(x)[mel * 20 + j], j < r
// What is moved off the chain:
//   teacher-forced: p and W_ih[:, 256:] p + b_ih of EVERY step (one GEMM before the launch,
//     `pre_gi`);
//   W_hh hA, W_hh h1, W_hh h2 (previous step's state) and W_ih[:, :256] ctx: computed right
//     after the vector they need has arrived, in the shadow of the next hand-off's wait.
// What stays: six all-to-all edges per step (hA, u, x, h1, h2, and — free-running only —
// the frames), each a vector every workgroup needs in full.
//
// Decomposition: 256 workgroups of 256 threads, one per CU (ftmi_resident_ok refuses the
// launch otherwise).  Workgroup g owns GRU unit g (3 gate rows of W_ih / W_hh), rows 2g, 2g+1
// of rnn_input, units 2g, 2g+1 of both LSTMs (8 gate rows of W_ih and W_hh each), tokens g
// and g + 256 of the attention energies, and the live mel_proj rows a = g, g + 256, ...
// (a = mel r + j -> row mel 20 + j: only 80 r of the 1600 rows are ever read).  Its 80 KB of
// weight rows are the same every step, so they stay in its XCD's L2 (2.5 MB per XCD) for the
// whole launch.  The softmax, the context vector, the query projection and (free-running) the
// prenet are small and computed redundantly by every workgroup from the gathered vectors:
// one edge less each.
//
// Arithmetic: exact fp32 FMAs, contraction off (the feedback and the stop test follow the
// fp32 reference), every sum in a fixed order.  A product over the workgroup's own rows is one
// wave's 64 lanes over float4 chunks of the row, met by shuffles (wave_dot); a product every
// workgroup computes in full reads the TRANSPOSED matrix with column-owning threads
// (cols_partial).  Measured: 44 us per step at T = 120 (args.stamps gives the
// per-phase sums).
//
// Hand-off: the data is the flag (rnn.hip, wavernn.hip; MI355X_MICROARCH.md, data-tagged
// granules): every exchanged value is one naturally aligned 8-byte {value, step + 1} granule
// written by ONE write-through (`sc1`) store and polled with `sc1` 8-byte loads until it
// carries the step's tag; two parity halves.  The workspace is zeroed by the call, so tag 0
// never matches.  Every spin is bounded: a timeout sets FTMI_STATUS_RNN_TIMEOUT in *status
// and the workgroup leaves, never a silent result.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TC_G = 256;     // workgroups (one per CU)
constexpr int TC_NT = 256;    // threads per workgroup
constexpr int TC_BMAX = FTMI_TACO_MAX_BATCH;
constexpr int TC_TMAX = FTMI_TACO_MAX_TOKENS;
constexpr int TC_D = 256;     // decoder_dims (= 2 encoder_dims: the context width)
constexpr int TC_H = 512;     // lstm_dims
constexpr int TC_P = 128;     // decoder prenet output
constexpr int TC_P1 = 256;    // decoder prenet hidden
constexpr int TC_NM = 80;     // n_mels
constexpr int TC_MAXR = 20;   // Decoder.max_r
constexpr int TC_NF = 32;     // LSA filters
constexpr int TC_KS = 31;     // LSA kernel size
constexpr int TC_PAD = 15;
constexpr int TC_MROWS = (TC_NM * TC_MAXR + TC_G - 1) / TC_G;  // live mel rows per workgroup
// granule offsets of the edges inside one (parity, batch item) block
constexpr int E_A = 0, E_U = E_A + TC_D, E_X = E_U + TC_TMAX, E_H1 = E_X + TC_H,
              E_H2 = E_H1 + TC_H, E_M = E_H2 + TC_H, E_END = E_M + TC_NM * TC_MAXR;
constexpr unsigned SPIN_LIMIT = 1u << 21;
constexpr unsigned STATUS_TIMEOUT = 4u;

typedef unsigned long long u64;

struct TcParams {
  ftmi_taco_args a;
  u64 *xch;
  int n_steps;  // decoder steps at most
  int free_run;
};

struct TcShared {
  __attribute__((aligned(16))) float ctx[TC_BMAX][TC_D];
  __attribute__((aligned(16))) float hA[TC_BMAX][TC_D];
  __attribute__((aligned(16))) float q[TC_BMAX][TC_D];
  __attribute__((aligned(16))) float x[TC_BMAX][TC_H];
  __attribute__((aligned(16))) float h1[TC_BMAX][TC_H];
  __attribute__((aligned(16))) float h2[TC_BMAX][TC_H];
  __attribute__((aligned(16))) float pre1[TC_BMAX][TC_P1];
  __attribute__((aligned(16))) float pre2[TC_BMAX][TC_P];
  // partial sums of the column-owned products: [k-part][item][column]
  __attribute__((aligned(16))) float part[TC_NT / (TC_P / 4) * TC_BMAX * TC_P];
  float u[TC_BMAX][TC_TMAX];
  float cumP[TC_BMAX][TC_TMAX + 2 * TC_PAD];  // zero-padded by the conv half-width
  float attP[TC_BMAX][TC_TMAX + 2 * TC_PAD];
  float mel[TC_NM * TC_MAXR];  // free-running (one item): the step's frames
  float mel_last[TC_NM];
  float convw[TC_NF * 2 * TC_KS];
  float convout[TC_NF];
  float red[4];
  float gictx[TC_BMAX][3], gipre[TC_BMAX][3], gh[TC_BMAX][3];
  float l_ih[TC_BMAX][8], l1_hh[TC_BMAX][8], l2_hh[TC_BMAX][8];
  float c1[TC_BMAX][2], c2[TC_BMAX][2];
  unsigned long long stamp[FTMI_TACO_STAMPS];  // diag phase sums (thread 0 of workgroup 0)
  int abort_flag;
};

__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + expf(-v)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// one wave: acc[b] = sum_k w[k] v[b][k] over n floats (n % 4 == 0, w and v 16-B aligned);
// lane l takes the float4 chunks l, l + 64, ...; every lane returns the sum
__device__ __forceinline__ void wave_dot(const float *__restrict__ w, const float *v, int vstride,
                                         int n, int B, float (&acc)[TC_BMAX]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int b = 0; b < TC_BMAX; ++b) acc[b] = 0.0f;
  for (int k4 = lane; k4 < (n >> 2); k4 += 64) {
    const f32x4 a = *reinterpret_cast<const f32x4 *>(w + 4 * k4);
#pragma unroll
    for (int b = 0; b < TC_BMAX; ++b)
      if (b < B) {
        const f32x4 xv = *reinterpret_cast<const f32x4 *>(v + b * vstride + 4 * k4);
        acc[b] = __builtin_fmaf(a.x, xv.x, acc[b]);
        acc[b] = __builtin_fmaf(a.y, xv.y, acc[b]);
        acc[b] = __builtin_fmaf(a.z, xv.z, acc[b]);
        acc[b] = __builtin_fmaf(a.w, xv.w, acc[b]);
      }
  }
#pragma unroll
  for (int b = 0; b < TC_BMAX; ++b) acc[b] = wave_sum(acc[b]);
}

// Products every workgroup computes in full (prenet, query projection, context): the matrix
// is given TRANSPOSED, wt [K][N] (N = 128 or 256).  A thread owns 4 adjacent columns and every
// PARTS-th k (PARTS = 256 / (N / 4)), so a wave's 16-B loads cover whole rows and 8 of them
// are in flight at once (one column per thread and a serial k loop cost a load latency per
// few k: 21 us for the 256 x 256 query projection); the k-parts meet in fixed order in
// colsum.  part[(k-part * TC_BMAX + b) * N + column].
template <int N>
__device__ __forceinline__ void cols_partial(const float *__restrict__ wt, int K, const float *v,
                                             int vstride, int B, float *part) {
  constexpr int C4 = N / 4, PARTS = TC_NT / C4;
  const int c4 = threadIdx.x % C4, pi = threadIdx.x / C4;
  f32x4 acc[TC_BMAX];
#pragma unroll
  for (int b = 0; b < TC_BMAX; ++b) acc[b] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 8
  for (int k = pi; k < K; k += PARTS) {
    const f32x4 w = *reinterpret_cast<const f32x4 *>(wt + (size_t)k * N + 4 * c4);
#pragma unroll
    for (int b = 0; b < TC_BMAX; ++b)
      if (b < B) {
        const float xv = v[b * vstride + k];
        acc[b].x = __builtin_fmaf(w.x, xv, acc[b].x);
        acc[b].y = __builtin_fmaf(w.y, xv, acc[b].y);
        acc[b].z = __builtin_fmaf(w.z, xv, acc[b].z);
        acc[b].w = __builtin_fmaf(w.w, xv, acc[b].w);
      }
  }
#pragma unroll
  for (int b = 0; b < TC_BMAX; ++b)
    if (b < B) *reinterpret_cast<f32x4 *>(part + ((pi * TC_BMAX + b) * N + 4 * c4)) = acc[b];
}
template <int N>
__device__ __forceinline__ float colsum(const float *part, int b, int n) {
  constexpr int PARTS = TC_NT / (N / 4);
  float v = part[b * N + n];
#pragma unroll
  for (int i = 1; i < PARTS; ++i) v += part[(i * TC_BMAX + b) * N + n];
  return v;
}

__device__ __forceinline__ u64 *granule(const TcParams &p, int s, int b, int edge_idx) {
  return p.xch + ((size_t)((s & 1) * TC_BMAX + b) * E_END + edge_idx);
}

__device__ __forceinline__ void publish(const TcParams &p, int s, int b, int edge_idx, float v) {
  const u64 g = ((u64)(unsigned)(s + 1) << 32) | (u64)__float_as_uint(v);
  __hip_atomic_store(granule(p, s, b, edge_idx), g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// gather n values per batch item of one edge into dst[b * dstride + k].  Every granule of the
// thread is requested at once, then only the stale ones are polled again.  Ends with a
// workgroup barrier; returns false (for every thread) when a spin ran out.
template <int PER>
__device__ __forceinline__ bool acquire(const TcParams &p, TcShared &sh, int s, int edge, int n,
                                        float *dst, int dstride) {
  const int tid = threadIdx.x;
  const int total = p.a.B * n;
  const unsigned want = (unsigned)(s + 1);
  u64 r[PER];
  unsigned stale = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i)
    if (tid + i * TC_NT < total) stale |= 1u << i;
  for (unsigned spins = 0; stale; ++spins) {
    asm volatile("" ::: "memory");  // the poll stores nothing: keep the loads in the loop
#pragma unroll
    for (int i = 0; i < PER; ++i)
      if (stale & (1u << i)) {
        const int idx = tid + i * TC_NT;
        const int b = idx / n, k = idx - b * n;
        r[i] = __hip_atomic_load(granule(p, s, b, edge + k), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
    for (int i = 0; i < PER; ++i)
      if ((stale & (1u << i)) && (unsigned)(r[i] >> 32) == want) {
        const int idx = tid + i * TC_NT;
        const int b = idx / n, k = idx - b * n;
        dst[b * dstride + k] = __uint_as_float((unsigned)r[i]);
        stale &= ~(1u << i);
      }
    if (stale) {
      if (spins > SPIN_LIMIT) {
        sh.abort_flag = 1;
        if (p.a.status) atomicOr(p.a.status, STATUS_TIMEOUT);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  __syncthreads();
  return sh.abort_flag == 0;
}

// W_hh h + b_ih + b_hh of the workgroup's 8 LSTM gate rows (gate i = row / 2, unit 2g + row % 2)
__device__ __forceinline__ void lstm_rows(const float *w, const float *bias_a, const float *bias_b,
                                          const float *vec, int B, float (*out)[8]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = blockIdx.x;
  for (int i = wave; i < 8; i += 4) {
    const int row = (i >> 1) * TC_H + 2 * g + (i & 1);
    float acc[TC_BMAX];
    wave_dot(w + (size_t)row * TC_H, vec, TC_H, TC_H, B, acc);
    if (lane == 0) {
      const float bs = bias_a ? bias_a[row] + bias_b[row] : 0.0f;
      for (int b = 0; b < B; ++b) out[b][i] = acc[b] + bs;
    }
  }
}

// the cell update of the workgroup's two units and the publication of their h
__device__ __forceinline__ void lstm_cell(const TcParams &p, TcShared &sh, int s, int edge,
                                          float (*hh)[8], float (*c)[2]) {
  const int tid = threadIdx.x, g = blockIdx.x;
  if (tid < 2 * p.a.B) {
    const int b = tid >> 1, uu = tid & 1;
    const float gi = sigm(sh.l_ih[b][0 + uu] + hh[b][0 + uu]);
    const float gf = sigm(sh.l_ih[b][2 + uu] + hh[b][2 + uu]);
    const float gg = tanhf(sh.l_ih[b][4 + uu] + hh[b][4 + uu]);
    const float go = sigm(sh.l_ih[b][6 + uu] + hh[b][6 + uu]);
    const float cn = gf * c[b][uu] + gi * gg;
    c[b][uu] = cn;
    publish(p, s, b, edge + 2 * g + uu, go * tanhf(cn));
  }
}

__global__ __launch_bounds__(TC_NT, 1) void taco_decoder_kernel(const TcParams p) {
  __shared__ TcShared sh;
  const ftmi_taco_args &a = p.a;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = blockIdx.x;
  const int B = a.B, T = a.T, r = a.r;
  const int n_live = TC_NM * r;  // live mel_proj rows

  for (int i = tid; i < (int)(sizeof(TcShared) / 4); i += TC_NT) reinterpret_cast<float *>(&sh)[i] = 0.0f;
  __syncthreads();
  for (int i = tid; i < TC_NF * 2 * TC_KS; i += TC_NT) sh.convw[i] = a.lsa_conv[i];
  // thread d keeps row d of LSA.L, its biases and v[d] for the whole launch
  float Lrow[TC_NF];
#pragma unroll
  for (int f = 0; f < TC_NF; ++f) Lrow[f] = a.lsa_L[tid * TC_NF + f];
  const float Lb = a.lsa_Lb[tid], Wb = a.lsa_Wb[tid], vd = a.lsa_v[tid];
  // ... and its tokens' enc_proj values (the same every step)
  float encp[TC_BMAX][(TC_TMAX + TC_G - 1) / TC_G];
#pragma unroll
  for (int b = 0; b < TC_BMAX; ++b)
#pragma unroll
    for (int i = 0; i < (TC_TMAX + TC_G - 1) / TC_G; ++i) {
      const int tok = g + i * TC_G;
      encp[b][i] = (b < B && tok < T) ? a.enc_proj[((size_t)b * T + tok) * TC_D + tid] : 0.0f;
    }
  __syncthreads();

  // products with the zero initial state: the biases
  if (wave < 3 && lane == 0)
    for (int b = 0; b < B; ++b) sh.gh[b][wave] = a.gru_bhh[wave * TC_D + g];
  if (tid < 8) {
    const int row = (tid >> 1) * TC_H + 2 * g + (tid & 1);
    for (int b = 0; b < B; ++b) {
      sh.l1_hh[b][tid] = 0.0f + (a.l1_bih[row] + a.l1_bhh[row]);
      sh.l2_hh[b][tid] = 0.0f + (a.l2_bih[row] + a.l2_bhh[row]);
    }
  }
  __syncthreads();

  // diag (args.stamps): thread 0 of workgroup 0 sums s_memtime deltas per phase; timing only
  const bool stamping = a.stamps != nullptr && g == 0 && tid == 0;
  unsigned long long last_stamp = stamping ? __builtin_amdgcn_s_memtime() : 0ull;
#define TC_STAMP(i)                                                  \
  do {                                                               \
    if (stamping) {                                                  \
      const unsigned long long now__ = __builtin_amdgcn_s_memtime(); \
      sh.stamp[i] += now__ - last_stamp;                             \
      last_stamp = now__;                                            \
    }                                                                \
  } while (0)
  int done = 0;
  for (int s = 0; s < p.n_steps; ++s) {
    // ---- the prenet's share of the attention GRU's input product -----------------------
    if (p.free_run) {
      cols_partial<TC_P1>(a.pre_w1t, TC_NM, sh.mel_last, 0, 1, sh.part);
      __syncthreads();
      sh.pre1[0][tid] = fmaxf(colsum<TC_P1>(sh.part, 0, tid) + a.pre_b1[tid], 0.0f);
      __syncthreads();
      cols_partial<TC_P>(a.pre_w2t, TC_P1, &sh.pre1[0][0], 0, 1, sh.part);
      __syncthreads();
      if (tid < TC_P) sh.pre2[0][tid] = fmaxf(colsum<TC_P>(sh.part, 0, tid) + a.pre_b2[tid], 0.0f);
      __syncthreads();
      if (wave < 3) {
        const int row = wave * TC_D + g;
        float acc[TC_BMAX];
        wave_dot(a.gru_wih + (size_t)row * (TC_D + TC_P) + TC_D, &sh.pre2[0][0], TC_P, TC_P, B, acc);
        if (lane == 0)
          for (int b = 0; b < B; ++b) sh.gipre[b][wave] = acc[b] + a.gru_bih[row];
      }
    } else if (tid < 3 * B) {
      const int b = tid / 3, gate = tid - 3 * b;
      sh.gipre[b][gate] = a.pre_gi[((size_t)b * p.n_steps + s) * (3 * TC_D) + gate * TC_D + g];
    }
    __syncthreads();
    TC_STAMP(0);
    // ---- attention GRU cell of unit g -----------------------------------------------------
    if (tid < B) {
      const int b = tid;
      const float gr = sigm((sh.gictx[b][0] + sh.gipre[b][0]) + sh.gh[b][0]);
      const float gz = sigm((sh.gictx[b][1] + sh.gipre[b][1]) + sh.gh[b][1]);
      const float gn = tanhf((sh.gictx[b][2] + sh.gipre[b][2]) + gr * sh.gh[b][2]);
      const float hp = sh.hA[b][g];
      publish(p, s, b, E_A + g, gn + gz * (hp - gn));
    }
    TC_STAMP(1);
    if (!acquire<(TC_BMAX * TC_D + TC_NT - 1) / TC_NT>(p, sh, s, E_A, TC_D, &sh.hA[0][0], TC_D)) return;

    TC_STAMP(2);
    // ---- location-sensitive attention: energies of the workgroup's tokens -----------------
    if (g < T) {
      cols_partial<TC_D>(a.lsa_wt, TC_D, &sh.hA[0][0], TC_D, B, sh.part);
      __syncthreads();
      for (int b = 0; b < B; ++b) sh.q[b][tid] = colsum<TC_D>(sh.part, b, tid) + Wb;
      TC_STAMP(3);
#pragma unroll
      for (int ti = 0; ti < (TC_TMAX + TC_G - 1) / TC_G; ++ti) {
        const int tok = g + ti * TC_G;
        if (tok >= T) break;
#pragma unroll
        for (int b = 0; b < TC_BMAX; ++b) {
          if (b >= B) break;
          {
            const int f = tid >> 3, part = tid & 7;
            float acc = 0.0f;
            for (int j = part; j < 2 * TC_KS; j += 8) {
              const int c = j >= TC_KS, k = j - c * TC_KS;
              const float lv = c ? sh.attP[b][tok + k] : sh.cumP[b][tok + k];
              acc = __builtin_fmaf(sh.convw[(f * 2 + c) * TC_KS + k], lv, acc);
            }
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            acc += __shfl_xor(acc, 4);
            if (part == 0) sh.convout[f] = acc;
          }
          __syncthreads();
          float pl = Lb;
#pragma unroll
          for (int f = 0; f < TC_NF; ++f) pl = __builtin_fmaf(Lrow[f], sh.convout[f], pl);
          const float e = vd * tanhf((sh.q[b][tid] + encp[b][ti]) + pl);
          const float ws = wave_sum(e);
          if (lane == 0) sh.red[wave] = ws;
          __syncthreads();
          if (tid == 0) publish(p, s, b, E_U + tok, (sh.red[0] + sh.red[1]) + (sh.red[2] + sh.red[3]));
        }
      }
    }
    TC_STAMP(4);
    // shadow of the wait: W_hh hA + b_hh for the next step
    if (wave < 3) {
      const int row = wave * TC_D + g;
      float acc[TC_BMAX];
      wave_dot(a.gru_whh + (size_t)row * TC_D, &sh.hA[0][0], TC_D, TC_D, B, acc);
      if (lane == 0)
        for (int b = 0; b < B; ++b) sh.gh[b][wave] = acc[b] + a.gru_bhh[row];
    }
    TC_STAMP(5);
    if (!acquire<(TC_BMAX * TC_TMAX + TC_NT - 1) / TC_NT>(p, sh, s, E_U, T, &sh.u[0][0], TC_TMAX)) return;

    TC_STAMP(6);
    // ---- softmax over the tokens, cumulative attention, context (every workgroup) ---------
    for (int b = 0; b < B; ++b) {
      float m = -INFINITY;
      for (int t = tid; t < T; t += TC_NT) m = fmaxf(m, sh.u[b][t]);
      m = wave_max(m);
      if (lane == 0) sh.red[wave] = m;
      __syncthreads();
      m = fmaxf(fmaxf(sh.red[0], sh.red[1]), fmaxf(sh.red[2], sh.red[3]));
      __syncthreads();
      float e[(TC_TMAX + TC_NT - 1) / TC_NT], sum = 0.0f;
#pragma unroll
      for (int i = 0; i < (TC_TMAX + TC_NT - 1) / TC_NT; ++i) {
        const int t = tid + i * TC_NT;
        e[i] = t < T ? expf(sh.u[b][t] - m) : 0.0f;
        sum += e[i];
      }
      sum = wave_sum(sum);
      if (lane == 0) sh.red[wave] = sum;
      __syncthreads();
      sum = (sh.red[0] + sh.red[1]) + (sh.red[2] + sh.red[3]);
#pragma unroll
      for (int i = 0; i < (TC_TMAX + TC_NT - 1) / TC_NT; ++i) {
        const int t = tid + i * TC_NT;
        if (t < T) {
          const float sc = e[i] / sum;
          sh.attP[b][TC_PAD + t] = sc;
          sh.cumP[b][TC_PAD + t] += sc;
          if (g == 0) a.attn_out[((size_t)b * p.n_steps + s) * T + t] = sc;
        }
      }
      __syncthreads();
    }
    TC_STAMP(7);
    for (int b = 0; b < B; ++b)  // enc of item b is the (transposed) matrix: [T][256]
      cols_partial<TC_D>(a.enc + (size_t)b * T * TC_D, T, &sh.attP[b][TC_PAD], 0, 1, sh.part + b * TC_D);
    __syncthreads();
    for (int b = 0; b < B; ++b) sh.ctx[b][tid] = colsum<TC_D>(sh.part, b, tid);
    __syncthreads();

    TC_STAMP(8);
    // ---- rnn_input rows 2g, 2g + 1 --------------------------------------------------------
    if (wave < 2) {
      const int row = 2 * g + wave;
      float a0[TC_BMAX], a1[TC_BMAX];
      wave_dot(a.rin_w + (size_t)row * TC_H, &sh.ctx[0][0], TC_D, TC_D, B, a0);
      wave_dot(a.rin_w + (size_t)row * TC_H + TC_D, &sh.hA[0][0], TC_D, TC_D, B, a1);
      if (lane == 0)
        for (int b = 0; b < B; ++b) publish(p, s, b, E_X + row, (a0[b] + a1[b]) + a.rin_b[row]);
    }
    // shadow: W_ih[:, :256] ctx for the next step
    if (wave < 3) {
      const int row = wave * TC_D + g;
      float acc[TC_BMAX];
      wave_dot(a.gru_wih + (size_t)row * (TC_D + TC_P), &sh.ctx[0][0], TC_D, TC_D, B, acc);
      if (lane == 0)
        for (int b = 0; b < B; ++b) sh.gictx[b][wave] = acc[b];
    }
    TC_STAMP(9);
    if (!acquire<(TC_BMAX * TC_H + TC_NT - 1) / TC_NT>(p, sh, s, E_X, TC_H, &sh.x[0][0], TC_H)) return;

    TC_STAMP(10);
    // ---- first residual LSTM --------------------------------------------------------------
    lstm_rows(a.l1_wih, nullptr, nullptr, &sh.x[0][0], B, sh.l_ih);
    __syncthreads();
    lstm_cell(p, sh, s, E_H1, sh.l1_hh, sh.c1);
    TC_STAMP(11);
    if (!acquire<(TC_BMAX * TC_H + TC_NT - 1) / TC_NT>(p, sh, s, E_H1, TC_H, &sh.h1[0][0], TC_H)) return;
    TC_STAMP(12);
    for (int i = tid; i < B * TC_H; i += TC_NT) (&sh.x[0][0])[i] += (&sh.h1[0][0])[i];
    __syncthreads();

    // ---- second residual LSTM -------------------------------------------------------------
    lstm_rows(a.l2_wih, nullptr, nullptr, &sh.x[0][0], B, sh.l_ih);
    __syncthreads();
    lstm_cell(p, sh, s, E_H2, sh.l2_hh, sh.c2);
    // shadow: W_hh h1 + biases for the next step
    lstm_rows(a.l1_whh, a.l1_bih, a.l1_bhh, &sh.h1[0][0], B, sh.l1_hh);
    TC_STAMP(13);
    if (!acquire<(TC_BMAX * TC_H + TC_NT - 1) / TC_NT>(p, sh, s, E_H2, TC_H, &sh.h2[0][0], TC_H)) return;
    TC_STAMP(14);
    for (int i = tid; i < B * TC_H; i += TC_NT) (&sh.x[0][0])[i] += (&sh.h2[0][0])[i];
    __syncthreads();

    // ---- the live mel_proj rows -----------------------------------------------------------
    for (int i = wave; i < TC_MROWS; i += 4) {
      const int av = g + i * TC_G;
      if (av >= n_live) break;
      const int mel = av / r, j = av - mel * r;
      float acc[TC_BMAX];
      wave_dot(a.mel_w + (size_t)(mel * TC_MAXR + j) * TC_H, &sh.x[0][0], TC_H, TC_H, B, acc);
      if (lane == 0)
        for (int b = 0; b < B; ++b) {
          a.mel_out[((size_t)b * p.n_steps * r + (size_t)s * r + j) * TC_NM + mel] = acc[b];
          if (p.free_run) publish(p, s, b, E_M + av, acc[b]);
        }
    }
    // shadow: W_hh h2 + biases for the next step
    lstm_rows(a.l2_whh, a.l2_bih, a.l2_bhh, &sh.h2[0][0], B, sh.l2_hh);
    TC_STAMP(15);
    done = s + 1;
    if (p.free_run) {
      if (!acquire<(TC_BMAX * TC_NM * TC_MAXR + TC_NT - 1) / TC_NT>(p, sh, s, E_M, n_live, sh.mel, 0))
        return;
      // the reference's stop rule: every value of the step's r frames below the threshold
      // and t > 10 (t counts frames); a NaN is "not below", as there
      int loud = 0;
      for (int i = tid; i < n_live; i += TC_NT) loud |= !(sh.mel[i] < a.stop_threshold);
      if (tid < TC_NM) sh.mel_last[tid] = sh.mel[tid * r + r - 1];
      const int any_loud = __syncthreads_or(loud);
      TC_STAMP(16);
      if (!any_loud && s * r > 10) break;
    } else {
      __syncthreads();
    }
  }
  if (stamping)
    for (int i = 0; i < FTMI_TACO_STAMPS; ++i) a.stamps[i] = sh.stamp[i];
#undef TC_STAMP
  if (g == 0 && tid == 0 && a.steps_out) *a.steps_out = done;
}

}  // namespace

extern "C" int64_t ftmi_tacotron_decoder_workspace_bytes(int32_t B, int32_t T) {
  if (B <= 0 || B > TC_BMAX || T <= 0 || T > TC_TMAX) return 0;
  return (int64_t)2 * TC_BMAX * E_END * 8;
}

extern "C" int ftmi_tacotron_decoder(const ftmi_taco_args *a, ftmi_stream_t stream) {
  if (!a) return FTMI_E_ARG;
  if (!a->enc || !a->enc_proj || !a->gru_wih || !a->gru_whh || !a->gru_bih || !a->gru_bhh ||
      !a->lsa_conv || !a->lsa_L || !a->lsa_Lb || !a->lsa_wt || !a->lsa_Wb || !a->lsa_v ||
      !a->rin_w || !a->rin_b || !a->l1_wih || !a->l1_whh || !a->l1_bih || !a->l1_bhh ||
      !a->l2_wih || !a->l2_whh || !a->l2_bih || !a->l2_bhh || !a->mel_w || !a->mel_out ||
      !a->attn_out || !a->workspace)
    return FTMI_E_ARG;
  if (a->B <= 0 || a->T <= 0 || a->steps <= 0 || a->r <= 0) return FTMI_E_ARG;
  if (a->decoder_dims != TC_D || a->lstm_dims != TC_H || a->n_mels != TC_NM ||
      a->prenet_dims != TC_P || a->r > TC_MAXR)
    return FTMI_E_UNSUPPORTED;
  if (a->T > TC_TMAX || a->B > TC_BMAX) return FTMI_E_UNSUPPORTED;
  const int free_run = a->pre_gi == nullptr;
  if (free_run) {
    if (!a->pre_w1t || !a->pre_b1 || !a->pre_w2t || !a->pre_b2 || !a->steps_out) return FTMI_E_ARG;
    if (a->B != 1) return FTMI_E_UNSUPPORTED;
  }
  if (!ftmi_aligned16(a->enc) || !ftmi_aligned16(a->gru_wih) || !ftmi_aligned16(a->gru_whh) ||
      !ftmi_aligned16(a->rin_w) || !ftmi_aligned16(a->l1_wih) || !ftmi_aligned16(a->l1_whh) ||
      !ftmi_aligned16(a->l2_wih) || !ftmi_aligned16(a->l2_whh) || !ftmi_aligned16(a->mel_w) ||
      !ftmi_aligned16(a->workspace))
    return FTMI_E_ALIGN;
  if (int rc = ftmi_resident_ok((const void *)taco_decoder_kernel, TC_G, TC_NT, 0)) return rc;
  hipStream_t s = ftmi_hs(stream);
  TcParams p;
  p.a = *a;
  p.xch = (u64 *)a->workspace;
  p.n_steps = (a->steps + a->r - 1) / a->r;
  p.free_run = free_run;
  hipError_t e = hipMemsetAsync(a->workspace, 0,
                                (size_t)ftmi_tacotron_decoder_workspace_bytes(a->B, a->T), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(taco_decoder_kernel, dim3(TC_G), dim3(TC_NT), 0, s, p);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}
