// Alignment-side kernels: durations and attention scores from a Tacotron attention matrix
// (utils/duration_extraction.py, utils/metrics.py of the reference).
//   align_dijkstra_kernel  shortest monotone path through 1 - att: the reference's grid DAG
//                          (right / down / down-right edges, weight = destination cell) as a
//                          three-predecessor fp64 dynamic programme on an anti-diagonal
//                          wavefront, then a backtrack that counts frames per token
//   align_count_kernel     per-row argmax + sequential jump repair + bincount
//   attention_score_kernel argmax adjacency and mean peak height
// and what train_tacotron.py:23-104 makes of the durations (extract_pitch_energy):
//   phoneme_features_kernel   per-token means of the frame energy and of the voiced pitch
//   nonzero_moments_kernel    count / mean / population std of the non-zero phoneme pitches
//   normalize_nonzero_kernel  (v - mean) / std on them, in place
// One workgroup per item; no workgroup waits on another; every loop bound is known at launch.
#include "common.h"

namespace {

constexpr int AL_TMAX = FTMI_TACO_MAX_TOKENS;  // columns: one thread each
constexpr int AL_WIN = 64;                     // backtrack window: AL_WIN diagonals x AL_WIN columns
constexpr int AL_LD = 16;                      // window loads in flight per thread
constexpr int AL_GRP = 8;                      // diagonals per branch-free group
constexpr int AL_NT = 1024, AL_NW = AL_NT / 64;  // count / score block: one wave per row
constexpr int AL_CHUNK = 1024;                 // rows whose argmax one LDS pass holds
enum { AL_DIAG = 0, AL_UP = 1, AL_LEFT = 2 };

__device__ __forceinline__ int al_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Bytes of direction workspace per item: one byte per cell, DIAGONAL-major (diagonal d at
// d * TS, column j at + j, TS = T rounded up to the wave width = the block size) so that a
// diagonal's stores are contiguous and every thread of the block owns a byte of every
// diagonal.  rows + T - 1 diagonals, plus the AL_GRP - 1 the last group may run past the end.
static inline int64_t al_item_bytes(int64_t rows, int64_t T) {
  return (rows + T + AL_GRP) * ((T + 63) & ~(int64_t)63);
}

// ---------------------------------------------------------------------------------------
// Thread j owns column j.  On diagonal d it holds cell (i, j), i = d - j.  Its predecessors:
//   up   (i-1, j)   = its own value of diagonal d-1 (a register)
//   left (i,   j-1) = thread j-1's value of diagonal d-1 (LDS, double-buffered by d & 1)
//   diag (i-1, j-1) = what it read as `left` on diagonal d-1 (a register)
// so a diagonal costs one LDS store, one LDS load and one barrier.  Cells outside
// [0, R) x [0, C) hold +inf.  Ties: diagonal, then up, then left (strict < in that order).
// The diagonals run in groups of AL_GRP with no branch inside a group: a thread without a
// cell loads a clamped address and stores a direction nobody reads, so the compiler can count
// the group's loads (issued one group ahead of their use) instead of draining them.
__global__ __launch_bounds__(AL_TMAX) void align_dijkstra_kernel(
    const float *__restrict__ att, int64_t ld_row, int64_t ld_item, int rows, int T,
    const int32_t *__restrict__ mel_len, const int32_t *__restrict__ x_len,
    int32_t *__restrict__ dur_out, double *__restrict__ cost_out, uint8_t *__restrict__ ws,
    int64_t ws_item) {
  __shared__ double s_d[2][AL_TMAX + 1];  // [d & 1][column + 1]; slot 0 = column -1 = +inf
  __shared__ int s_dur[AL_TMAX];
  __shared__ uint8_t s_win[AL_WIN * AL_WIN];
  __shared__ int s_pos[3];  // backtrack position (i, j) and the done flag

  const int b = blockIdx.x, j = threadIdx.x, nt = blockDim.x;  // nt = TS
  const int R = al_clamp(mel_len[b], 1, rows);
  const int C = al_clamp(x_len ? x_len[b] : T, 1, T);
  const float *a = att + (int64_t)b * ld_item;
  uint8_t *dir = ws + (int64_t)b * ws_item;
  const double inf = __builtin_huge_val();
  const int nd = R + C - 1;  // diagonals 0 .. nd - 1

  for (int k = j; k < AL_TMAX; k += nt) s_dur[k] = 0;
  double own = j == 0 ? 0.0 : inf;  // D on diagonal 0: cell (0, 0) = 0, w[0][0] not counted
  double dg = inf;
  double cost = own;
  s_d[0][j + 1] = own;
  if (j == 0) s_d[0][0] = s_d[1][0] = inf;
  __syncthreads();

  // att at this thread's cell of diagonal d, the address clamped into [0, R) x [0, C)
  const float *col = a + min(j, C - 1);
  auto load = [&](int d) -> float { return col[(int64_t)al_clamp(d - j, 0, R - 1) * ld_row]; };
  float wn[AL_GRP];
#pragma unroll
  for (int k = 0; k < AL_GRP; ++k) wn[k] = load(1 + k);
  for (int d0 = 1; d0 < nd; d0 += AL_GRP) {
    float wc[AL_GRP];
#pragma unroll
    for (int k = 0; k < AL_GRP; ++k) wc[k] = wn[k];
#pragma unroll
    for (int k = 0; k < AL_GRP; ++k) wn[k] = load(d0 + AL_GRP + k);  // in flight during this group
#pragma unroll
    for (int k = 0; k < AL_GRP; ++k) {
      const int d = d0 + k, i = d - j;  // d may pass nd - 1: no thread has a cell there
      const double lf = s_d[(d - 1) & 1][j];
      const bool cell = j < C && i >= 0 && i < R;
      double m = dg;
      int c = AL_DIAG;
      if (own < m) { m = own; c = AL_UP; }
      if (lf < m) { m = lf; c = AL_LEFT; }
      // fp32 subtraction, fp64 add: numpy on the fp32 attention
      const double v = cell ? (double)(1.0f - wc[k]) + m : inf;
      dir[(int64_t)d * nt + j] = (uint8_t)c;
      s_d[d & 1][j + 1] = v;
      dg = lf;
      own = v;
      cost = d == nd - 1 ? v : cost;
      __syncthreads();
    }
  }
  if (j == C - 1 && cost_out) cost_out[b] = cost;  // column C - 1's last cell is (R - 1, C - 1)

  // ---- backtrack from (R - 1, C - 1): the block stages a window of directions in LDS
  // (AL_WIN diagonals back, AL_WIN columns left of the position), thread 0 walks it.  A step
  // lowers the diagonal by 1 or 2 and the column by 0 or 1, so a window lasts >= AL_WIN / 2
  // steps and (R + C) / (AL_WIN / 2) + 2 windows reach row 0.  Row i's frame goes to the
  // largest column the path visits in it: the column at which the walk enters the row.
  if (j == 0) {
    s_pos[0] = R - 1;
    s_pos[1] = C - 1;
    s_pos[2] = R == 1;
    s_dur[C - 1] = 1;
  }
  __syncthreads();
  const int max_win = (R + C) / (AL_WIN / 2) + 2;
  for (int w = 0; w < max_win; ++w) {
    const int pi = s_pos[0], pj = s_pos[1];
    if (s_pos[2]) break;  // uniform: read after a barrier
    const int dh = pi + pj;
    // AL_LD loads in flight per thread, no branch: a cell before diagonal 1 or column 0 is
    // never stepped from, so its slot takes the byte of the clamped address
    for (int base = j; base < AL_WIN * AL_WIN; base += AL_LD * nt) {
      uint8_t v[AL_LD];
#pragma unroll
      for (int u = 0; u < AL_LD; ++u) {
        const int idx = min(base + u * nt, AL_WIN * AL_WIN - 1);
        v[u] = dir[(int64_t)max(dh - (idx >> 6), 1) * nt + max(pj - (idx & 63), 0)];
      }
#pragma unroll
      for (int u = 0; u < AL_LD; ++u)
        if (base + u * nt < AL_WIN * AL_WIN) s_win[base + u * nt] = v[u];
    }
    __syncthreads();
    if (j == 0) {
      int i = pi, c = pj;
      for (int step = 0; step < 2 * AL_WIN; ++step) {
        if (i == 0 || dh - (i + c) >= AL_WIN || pj - c >= AL_WIN) break;
        int m = s_win[(dh - (i + c)) * AL_WIN + (pj - c)];
        if (c == 0) m = AL_UP;  // column 0 has one predecessor; also keeps c >= 0 whatever the byte
        if (m == AL_LEFT) {
          c -= 1;
        } else {
          i -= 1;
          if (m == AL_DIAG) c -= 1;
          s_dur[c] += 1;
        }
      }
      s_pos[0] = i;
      s_pos[1] = c;
      s_pos[2] = i == 0;
    }
    __syncthreads();
  }
  if (j < T) dur_out[(int64_t)b * T + j] = j < C ? s_dur[j] : 0;
}

// ---------------------------------------------------------------------------------------
// One wave: first-index argmax of row[0 .. n): (largest value, smallest index among equals).
__device__ __forceinline__ void al_row_argmax(const float *__restrict__ row, int n, int lane,
                                              float &best, int &arg) {
  float v = -__builtin_huge_valf();
  int ix = 0x7fffffff;
  for (int c = lane; c < n; c += 64) {
    const float x = row[c];
    if (x > v || ix == 0x7fffffff) { v = x; ix = c; }  // ascending c: the first maximum stays
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(ix, o, 64);
    if (i2 != 0x7fffffff && (ix == 0x7fffffff || v2 > v || (v2 == v && i2 < ix))) { v = v2; ix = i2; }
  }
  best = v;
  arg = ix;
}

// extract_durations_per_count: argmax over the first C columns, jump repair against the
// repaired predecessor, bincount of the first R rows.  Rows >= R cannot reach the count (the
// repair only looks back), so they are not read.
__global__ __launch_bounds__(AL_NT) void align_count_kernel(
    const float *__restrict__ att, int64_t ld_row, int64_t ld_item, int rows, int T,
    const int32_t *__restrict__ mel_len, const int32_t *__restrict__ x_len,
    int32_t *__restrict__ dur_out) {
  __shared__ int s_arg[AL_CHUNK];
  __shared__ int s_dur[AL_TMAX];
  __shared__ int s_prev;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = al_clamp(mel_len[b], 1, rows);
  const int C = al_clamp(x_len ? x_len[b] : T, 1, T);
  const float *a = att + (int64_t)b * ld_item;
  for (int k = tid; k < AL_TMAX; k += AL_NT) s_dur[k] = 0;
  if (tid == 0) s_prev = -1;
  __syncthreads();
  for (int t0 = 0; t0 < R; t0 += AL_CHUNK) {
    const int n = min(AL_CHUNK, R - t0);
    for (int t = wave; t < n; t += AL_NW) {
      float v;
      int ix;
      al_row_argmax(a + (int64_t)(t0 + t) * ld_row, C, lane, v, ix);
      if (lane == 0) s_arg[t] = ix;
    }
    __syncthreads();
    if (tid == 0) {  // the carried dependency: serial over the chunk
      int prev = s_prev;
      for (int t = 0; t < n; ++t) {
        int cur = s_arg[t];
        if (prev >= 0 && abs(cur - prev) > 10) cur = prev;
        s_arg[t] = cur;
        prev = cur;
      }
      s_prev = prev;
    }
    __syncthreads();
    for (int t = tid; t < n; t += AL_NT) atomicAdd(&s_dur[al_clamp(s_arg[t], 0, C - 1)], 1);
    __syncthreads();
  }
  for (int k = tid; k < T; k += AL_NT) dur_out[(int64_t)b * T + k] = k < C ? s_dur[k] : 0;
}

// attention_score: L = mel_len / r, n = min(rows, L) rows take part.
//   loc   = #{1 <= t < n : |a[t] - a[t-1]| <= r} / (L - 1)   (fp32 quotient of two integers;
//           computed in fp64 and rounded once, which is the correctly rounded fp32 quotient)
//   sharp = (sum_{t < n} max_j att[t][j]) / rows, the sum in fp64 in a fixed order
__global__ __launch_bounds__(AL_NT) void attention_score_kernel(
    const float *__restrict__ att, int64_t ld_row, int64_t ld_item, int rows, int T,
    const int32_t *__restrict__ mel_len, int r, float *__restrict__ loc_out,
    float *__restrict__ sharp_out) {
  __shared__ int s_arg[AL_CHUNK + 1];  // [0]: the row before the chunk
  __shared__ double s_sum[AL_NW];
  __shared__ int s_cnt[AL_NW];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = mel_len[b] / r;
  const int n = al_clamp(L, 0, rows);
  const float *a = att + (int64_t)b * ld_item;
  double sum = 0.0;  // lane 0 of each wave: its rows' maxima
  int cnt = 0;
  for (int t0 = 0; t0 < n; t0 += AL_CHUNK) {
    const int m = min(AL_CHUNK, n - t0);
    for (int t = wave; t < m; t += AL_NW) {
      float v;
      int ix;
      al_row_argmax(a + (int64_t)(t0 + t) * ld_row, T, lane, v, ix);
      if (lane == 0) {
        s_arg[t + 1] = ix;
        sum += (double)v;
      }
    }
    __syncthreads();
    for (int t = tid; t < m; t += AL_NT)
      if (t0 + t >= 1 && abs(s_arg[t + 1] - s_arg[t]) <= r) cnt += 1;
    __syncthreads();
    if (tid == 0) s_arg[0] = s_arg[m];
    __syncthreads();
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if (lane == 0) {
    s_sum[wave] = sum;
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;  // a fixed order: the same bits on every launch
    int c = 0;
    for (int w = 0; w < AL_NW; ++w) {
      s += s_sum[w];
      c += s_cnt[w];
    }
    if (loc_out) loc_out[b] = (float)((double)c / (double)(L - 1));
    if (sharp_out) sharp_out[b] = (float)(s / (double)rows);
  }
}

int al_check(const float *att, int64_t ld_row, int64_t ld_item, int32_t B, int32_t rows, int32_t T,
             const int32_t *mel_len) {
  if (!att || !mel_len) return FTMI_E_ARG;
  if (B <= 0 || rows <= 0 || T <= 0) return FTMI_E_ARG;
  if (T > AL_TMAX) return FTMI_E_UNSUPPORTED;
  if (ld_row < T || ld_item < 0) return FTMI_E_SHAPE;
  if (((uintptr_t)att & 3u) || ((uintptr_t)mel_len & 3u)) return FTMI_E_ALIGN;
  return FTMI_OK;
}

// ---------------------------------------------------------------------------------------
// Phoneme-level pitch and energy (train_tacotron.py:37-104).  Frames pass through LDS in chunks
// of PF_CHUNK: a thread per frame computes energy[t] = sqrt(sum_k exp(mel[k][t])^2) in fp64 (for
// a fixed bin the loads of a wave are contiguous along t) and stages the frame's pitch, then a
// thread per token adds the chunk's part of its frame range [cum[i], cum[i+1]) to its running
// fp64 sums, in t order.  Nothing here depends on B or on which chunk a frame falls in, so an
// item's result is the same bits in every batch.
constexpr int PF_NT = 1024;    // >= 2 * AL_TMAX: a thread per token, two frames per thread and chunk
constexpr int PF_NW = PF_NT / 64;
constexpr int PF_CHUNK = 2048;  // frames per LDS pass: 8 B energy + 4 B pitch each
constexpr int PF_KU = 8;        // mel loads in flight per thread

__global__ __launch_bounds__(PF_NT) void phoneme_features_kernel(
    const float *__restrict__ mel, int64_t ld_bin, int64_t ld_item, int n_mels, int rows,
    const int32_t *__restrict__ mel_len, const int32_t *__restrict__ dur, int64_t ld_dur, int T,
    const int32_t *__restrict__ x_len, const float *__restrict__ pitch, int64_t ld_pitch, int P,
    const int32_t *__restrict__ pitch_len, float pitch_max_freq, float *__restrict__ pitch_out,
    float *__restrict__ energy_out, int32_t *__restrict__ dur_sum) {
  __shared__ double s_e[PF_CHUNK];
  __shared__ float s_p[PF_CHUNK];
  __shared__ long long s_w[2][PF_NW];  // per wave: sum of the clamped durations, of the raw ones
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = al_clamp(mel_len[b], 0, rows);
  const int C = al_clamp(x_len ? x_len[b] : T, 0, T);
  const int PL = pitch ? al_clamp(pitch_len[b], 0, P) : 0;
  const int ntok = min(C, L);  // the reference's loop zips over range(mel_len)

  // cum[i], cum[i + 1] of token i = tid: a block scan of max(dur, 0) over the first C columns
  // (int64: no duration array overflows it); the raw sum is what the host compares with mel_len
  const int d = dur[(int64_t)b * ld_dur + min(tid, T - 1)];
  long long dc = tid < C ? max(d, 0) : 0, dr = tid < C ? d : 0;
  const long long own = dc;
  for (int o = 1; o < 64; o <<= 1) {
    const long long uc = __shfl_up(dc, o, 64), ur = __shfl_up(dr, o, 64);
    if (lane >= o) { dc += uc; dr += ur; }
  }
  if (lane == 63) { s_w[0][wave] = dc; s_w[1][wave] = dr; }
  __syncthreads();
  long long raw = 0;
  for (int w = 0; w < PF_NW; ++w) {
    if (w < wave) dc += s_w[0][w];
    raw += s_w[1][w];
  }
  if (tid == 0) dur_sum[b] = (int32_t)(raw > 0x7fffffffLL ? 0x7fffffffLL : (raw < -0x80000000LL ? -0x80000000LL : raw));
  const int fb = (int)(dc < L ? dc : L);                // frame range [fa, fb), clamped to mel_len
  const int fa = (int)(dc - own < L ? dc - own : L);

  const float *m = mel + (int64_t)b * ld_item;
  const float *pb = pitch ? pitch + (int64_t)b * ld_pitch : nullptr;
  double es = 0.0, ps = 0.0;
  int pc = 0;
  for (int c0 = 0; c0 < L; c0 += PF_CHUNK) {
    const int n = min(PF_CHUNK, L - c0);
    for (int f = tid; f < n; f += PF_NT) {
      const int t = c0 + f;  // < L <= rows
      double s = 0.0;
      for (int k0 = 0; k0 < n_mels; k0 += PF_KU) {
        float v[PF_KU];  // no branch around a load: the bin index is clamped, the sum is masked
#pragma unroll
        for (int u = 0; u < PF_KU; ++u) v[u] = m[(int64_t)min(k0 + u, n_mels - 1) * ld_bin + t];
#pragma unroll
        for (int u = 0; u < PF_KU; ++u) {
          const double e = exp((double)v[u]);
          s = k0 + u < n_mels ? __dadd_rn(s, __dmul_rn(e, e)) : s;
        }
      }
      s_e[f] = sqrt(s);
      if (pb) {
        const float pv = pb[min(t, max(PL - 1, 0))];
        s_p[f] = t < PL ? pv : 0.0f;  // 0: never kept
      }
    }
    __syncthreads();
    if (tid < ntok) {
      const int lo = max(fa, c0) - c0, hi = min(fb, c0 + n) - c0;
      for (int f = lo; f < hi; ++f) {
        es += s_e[f];
        if (pb) {
          const float pv = s_p[f];
          if (pv != 0.0f && pv < pitch_max_freq) { ps += (double)pv; pc += 1; }
        }
      }
    }
    __syncthreads();
  }
  if (tid < T) {
    const bool live = tid < ntok;
    energy_out[(int64_t)b * T + tid] = live && fb > fa ? (float)(es / (double)(fb - fa)) : 0.0f;
    if (pb) pitch_out[(int64_t)b * T + tid] = live && pc > 0 ? (float)(ps / (double)pc) : 0.0f;
  }
}

// Count, mean and population standard deviation of the non-zero entries of v[0 .. n), fp64, two
// passes (sum (v - mean)^2, like np.std).  One workgroup: thread i adds entries i, i + MO_NT, ...
// in that order, and the MO_NT partials meet in a fixed tree, so the result repeats bit for bit.
constexpr int MO_NT = 1024;
constexpr int MO_U = 8;  // loads in flight per thread

__device__ __forceinline__ double mo_block_sum(double v, double *s, int tid) {
  __syncthreads();  // s may still be read from the previous sum
  s[tid] = v;
  __syncthreads();
  for (int o = MO_NT / 2; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  return s[0];
}

__global__ __launch_bounds__(MO_NT) void nonzero_moments_kernel(const float *__restrict__ v,
                                                                int64_t n, double *__restrict__ out) {
  __shared__ double s_red[MO_NT];
  const int tid = threadIdx.x;
  double cnt = 0.0, sum = 0.0;  // a count below 2^53 is exact in fp64
  for (int64_t i0 = tid; i0 < n; i0 += (int64_t)MO_NT * MO_U) {
    float x[MO_U];
#pragma unroll
    for (int u = 0; u < MO_U; ++u) x[u] = v[min(i0 + (int64_t)u * MO_NT, n - 1)];
#pragma unroll
    for (int u = 0; u < MO_U; ++u)
      if (i0 + (int64_t)u * MO_NT < n && x[u] != 0.0f) { cnt += 1.0; sum += (double)x[u]; }
  }
  cnt = mo_block_sum(cnt, s_red, tid);
  sum = mo_block_sum(sum, s_red, tid);
  const double mean = cnt > 0.0 ? sum / cnt : 0.0;
  double sq = 0.0;
  for (int64_t i0 = tid; i0 < n; i0 += (int64_t)MO_NT * MO_U) {
    float x[MO_U];
#pragma unroll
    for (int u = 0; u < MO_U; ++u) x[u] = v[min(i0 + (int64_t)u * MO_NT, n - 1)];
#pragma unroll
    for (int u = 0; u < MO_U; ++u)
      if (i0 + (int64_t)u * MO_NT < n && x[u] != 0.0f) {
        const double dv = (double)x[u] - mean;
        sq = __dadd_rn(sq, __dmul_rn(dv, dv));
      }
  }
  sq = mo_block_sum(sq, s_red, tid);
  if (tid == 0) {
    out[0] = cnt;
    out[1] = mean;
    out[2] = cnt > 0.0 ? sqrt(sq / cnt) : 0.0;
  }
}

// v = (v - mean) / std where v != 0: an fp32 subtraction, then the correctly rounded fp32
// quotient, which is what numpy's `v -= mean; v /= std` computes.
__global__ __launch_bounds__(256) void normalize_nonzero_kernel(float *__restrict__ v, int64_t n,
                                                                float mean, float std) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
    const float x = v[i];
    if (x != 0.0f) v[i] = __fdiv_rn(__fsub_rn(x, mean), std);
  }
}

}  // namespace

extern "C" int64_t ftmi_align_workspace_bytes(int32_t B, int32_t rows, int32_t T) {
  if (B <= 0 || rows <= 0 || T <= 0 || T > AL_TMAX) return 0;
  return (int64_t)B * al_item_bytes(rows, T);
}

extern "C" int ftmi_align_dijkstra(const float *att, int64_t ld_row, int64_t ld_item, int32_t B,
                                   int32_t rows, int32_t T, const int32_t *mel_len,
                                   const int32_t *x_len, int32_t *dur_out, double *cost_out,
                                   void *workspace, ftmi_stream_t stream) {
  const int rc = al_check(att, ld_row, ld_item, B, rows, T, mel_len);
  if (rc) return rc;
  if (!dur_out || !workspace) return FTMI_E_ARG;
  if (((uintptr_t)x_len & 3u) || ((uintptr_t)dur_out & 3u) || ((uintptr_t)cost_out & 7u) ||
      !ftmi_aligned16(workspace))
    return FTMI_E_ALIGN;
  const int nt = (T + 63) & ~63;
  hipLaunchKernelGGL(align_dijkstra_kernel, dim3(B), dim3(nt), 0, ftmi_hs(stream), att, ld_row,
                     ld_item, rows, T, mel_len, x_len, dur_out, cost_out, (uint8_t *)workspace,
                     al_item_bytes(rows, T));
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int ftmi_align_count(const float *att, int64_t ld_row, int64_t ld_item, int32_t B,
                                int32_t rows, int32_t T, const int32_t *mel_len,
                                const int32_t *x_len, int32_t *dur_out, ftmi_stream_t stream) {
  const int rc = al_check(att, ld_row, ld_item, B, rows, T, mel_len);
  if (rc) return rc;
  if (!dur_out) return FTMI_E_ARG;
  if (((uintptr_t)x_len & 3u) || ((uintptr_t)dur_out & 3u)) return FTMI_E_ALIGN;
  hipLaunchKernelGGL(align_count_kernel, dim3(B), dim3(AL_NT), 0, ftmi_hs(stream), att, ld_row,
                     ld_item, rows, T, mel_len, x_len, dur_out);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int ftmi_attention_score(const float *att, int64_t ld_row, int64_t ld_item, int32_t B,
                                    int32_t rows, int32_t T, const int32_t *mel_len, int32_t r,
                                    float *loc_out, float *sharp_out, ftmi_stream_t stream) {
  const int rc = al_check(att, ld_row, ld_item, B, rows, T, mel_len);
  if (rc) return rc;
  if (r <= 0 || (!loc_out && !sharp_out)) return FTMI_E_ARG;
  if (((uintptr_t)loc_out & 3u) || ((uintptr_t)sharp_out & 3u)) return FTMI_E_ALIGN;
  hipLaunchKernelGGL(attention_score_kernel, dim3(B), dim3(AL_NT), 0, ftmi_hs(stream), att, ld_row,
                     ld_item, rows, T, mel_len, r, loc_out, sharp_out);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int ftmi_phoneme_features(const float *mel, int64_t ld_bin, int64_t ld_item, int32_t B,
                                     int32_t n_mels, int32_t rows, const int32_t *mel_len,
                                     const int32_t *dur, int64_t ld_dur, int32_t T,
                                     const int32_t *x_len, const float *pitch, int64_t ld_pitch,
                                     int32_t P, const int32_t *pitch_len, float pitch_max_freq,
                                     float *pitch_out, float *energy_out, int32_t *dur_sum,
                                     ftmi_stream_t stream) {
  if (!mel || !mel_len || !dur || !energy_out || !dur_sum) return FTMI_E_ARG;
  if (B <= 0 || n_mels <= 0 || rows <= 0 || T <= 0) return FTMI_E_ARG;
  if ((pitch != nullptr) != (pitch_len != nullptr) || (pitch != nullptr) != (pitch_out != nullptr))
    return FTMI_E_ARG;  // pitch, its lengths and its output come together or not at all
  if (pitch && P <= 0) return FTMI_E_ARG;
  if (T > AL_TMAX) return FTMI_E_UNSUPPORTED;
  if (ld_bin < rows || ld_item < 0 || ld_dur < T || (pitch && ld_pitch < P)) return FTMI_E_SHAPE;
  if (((uintptr_t)mel | (uintptr_t)mel_len | (uintptr_t)dur | (uintptr_t)x_len | (uintptr_t)pitch |
       (uintptr_t)pitch_len | (uintptr_t)pitch_out | (uintptr_t)energy_out | (uintptr_t)dur_sum) & 3u)
    return FTMI_E_ALIGN;
  hipLaunchKernelGGL(phoneme_features_kernel, dim3(B), dim3(PF_NT), 0, ftmi_hs(stream), mel, ld_bin,
                     ld_item, n_mels, rows, mel_len, dur, ld_dur, T, x_len, pitch, ld_pitch, P,
                     pitch_len, pitch_max_freq, pitch_out, energy_out, dur_sum);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int ftmi_nonzero_moments(const float *values, int64_t n, double *out,
                                    ftmi_stream_t stream) {
  if (!values || !out || n <= 0) return FTMI_E_ARG;
  if (((uintptr_t)values & 3u) || ((uintptr_t)out & 7u)) return FTMI_E_ALIGN;
  hipLaunchKernelGGL(nonzero_moments_kernel, dim3(1), dim3(MO_NT), 0, ftmi_hs(stream), values, n, out);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}

extern "C" int ftmi_normalize_nonzero(float *values, int64_t n, float mean, float std,
                                      ftmi_stream_t stream) {
  if (!values || n <= 0) return FTMI_E_ARG;
  if ((uintptr_t)values & 3u) return FTMI_E_ALIGN;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(normalize_nonzero_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)),
                     dim3(256), 0, ftmi_hs(stream), values, n, mean, std);
  FTMI_CHECK_LAUNCH();
  return FTMI_OK;
}
