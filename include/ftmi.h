/*
 * ftmi.h — C ABI of libftmi.so, the MI355X (gfx950) hot path of ForwardTacotron
 * inference (reference: tarepan/ForwardTacotron, models/forward_tacotron.py).
 *
 * Every entry point:
 *   - works on CALLER-OWNED device buffers (plain pointers + sizes, fp32 unless stated);
 *   - enqueues on the given HIP stream (ftmi_stream_t = hipStream_t, NULL = null stream)
 *     and never synchronises, allocates or frees;
 *   - returns 0 on success, an FTMI_E_* code (>= 1000) for argument / shape errors
 *     detected on the host, or a hipError_t (< 1000) if a launch failed.
 *
 * Layout convention: sequences are CHANNELS-LAST, (B, T, C) rows of C floats with a
 * row stride given in floats. The reference's (B, C, T) tensors are produced only at
 * the API edge (mel / mel_post outputs) through the transposed-store option.
 *
 * Each function names the reference code it replaces (file:line in the reference).
 */
#ifndef FTMI_H
#define FTMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *ftmi_stream_t; /* hipStream_t */

enum {
  FTMI_OK = 0,
  FTMI_E_ARG = 1001,         /* null pointer / non-positive size */
  FTMI_E_SHAPE = 1002,       /* shape constraint violated (e.g. Cin % 16 != 0) */
  FTMI_E_UNSUPPORTED = 1003, /* configuration without a compiled kernel */
  FTMI_E_ALIGN = 1004        /* pointer / stride not 16-byte aligned */
};

/* Matrix-core path of the dense contractions (conv1d / conv_bank / highway):
 *   FTMI_MMA_F32     v_mfma_f32_32x32x2_f32: exact fp32 products, 157 TFLOP/s peak.
 *   FTMI_MMA_BF16X6  each fp32 operand split into three bf16 pieces (a = a1+a2+a3, exact),
 *                    the six cross products with i+j <= 4 on v_mfma_f32_16x16x32_bf16 with
 *                    fp32 accumulation: fp32-accurate (dropped terms < 2^-24 relative) at
 *                    16/6 of the fp32 MFMA rate.
 *   FTMI_MMA_F16X3   (default) each operand split into an f16 head and a 2^11-scaled f16
 *                    tail; weights pre-split by ftmi_split_weights_f16 (three f16 planes
 *                    + a power-of-two column scale); three v_mfma_f32_16x16x32_f16 per
 *                    product, fp32 accumulation: fp32-level accuracy (dropped terms
 *                    < 2^-22 relative) at 16/3 of the fp32 MFMA rate.  Activations must
 *                    stay below 65504 in magnitude: otherwise the output is invalid and
 *                    bit 0 of *status (optional) is set — recompute on FTMI_MMA_F32. */
enum { FTMI_MMA_F32 = 0, FTMI_MMA_BF16X6 = 1, FTMI_MMA_F16X3 = 2 };

/* Bits of the optional device status word (uint32_t *status) the kernels OR into; the
 * caller zeroes it, runs, and reads it once after the stream completed:
 *   FTMI_STATUS_F16_RANGE    an f16x3 GEMM saw an activation beyond the f16 range (its
 *                            output is invalid: recompute on FTMI_MMA_F32)
 *   FTMI_STATUS_WHH_RANGE    a recurrence's W_hh entry is beyond the f16 range (idem)
 *   FTMI_STATUS_RNN_TIMEOUT  a recurrence workgroup gave up waiting for its group (not all
 *                            workgroups co-resident): the output is invalid — an error,
 *                            not a precision event */
enum { FTMI_STATUS_F16_RANGE = 1, FTMI_STATUS_WHH_RANGE = 2, FTMI_STATUS_RNN_TIMEOUT = 4 };

/* ftmi_conv_bank_split pool_out flags (ABI 10; 0 / 1 keep their ABI 9 meaning) */
enum { FTMI_BANK_POOL = 1,    /* y = CBHG maxpool(2, 1) of the bank output */
       FTMI_BANK_Y_SPLIT = 2, /* with FTMI_BANK_POOL: y as f16x3 split rows of K*Cout */
       FTMI_BANK_X_SPLIT = 4, /* x given as f16x3 split rows of Cin (FTMI_MMA_F16X3) */
       FTMI_BANK_HALVES = 16, /* ABI 15 (alone, FTMI_MMA_F16X3): the few-row bank in ONE
                                 launch — a block per (group pair, 16-column set, half of the
                                 input channels), each wave's weight stream issued at once, the
                                 unit's two halves combined in-kernel by the last to arrive
                                 (deterministic).  B*T <= 128, Cin % 64 == 0, Cin <= 256, K even,
                                 (K / 2)(Cout / 16) % 8 == 0 and <= 512; else FTMI_E_UNSUPPORTED.  split_ws:
                                 ftmi_conv_bank_halves_ws_floats(B, T, K, Cout) floats, the first
                                 FTMI_BANK_COUNTERS zeroed once by the caller (every launch leaves
                                 them zero); split_k is ignored.  One workspace per stream. */
       FTMI_BANK_IMAGE = 32   /* ABI 16, with FTMI_BANK_HALVES: w_split is the bank's
                                 stream-order weight image (ftmi_conv_bank_halves_image), which
                                 the kernel reads as one contiguous 1 KB run per wave load;
                                 same results bit for bit. */ };
enum { FTMI_BANK_COUNTERS = 4096 };

/* ABI version; bumped on any signature change (14: ftmi_panel_proj_qkv, ftmi_attention_kv;
 * 15: FTMI_BANK_HALVES, ftmi_conv_bank_halves_ws_floats; 16: FTMI_BANK_IMAGE,
 * ftmi_conv_bank_halves_image[_bytes]; 17: FTMI_BANK_PAIR, ftmi_conv_args.x_plane / x_fin;
 * 18: rejected variants removed — FTMI_BANK_LAST, FTMI_BANK_PAIR, ftmi_conv_args.x_plane /
 * x_fin, ftmi_gru_bidir_fused; ftmi_highway_stack_spread[_ws_bytes|_blocks] added;
 * 19: ftmi_nnls_lbfgsb_*, ftmi_set_resident_cu_limit, the persistent-launch guard,
 * ftmi_griffinlim_iter, ftmi_istft_fused; 20: ftmi_tacotron_decoder[_workspace_bytes];
 * added under 20 without a signature change: ftmi_align_workspace_bytes,
 * ftmi_align_dijkstra, ftmi_align_count, ftmi_attention_score; ftmi_phoneme_features,
 * ftmi_nonzero_moments, ftmi_normalize_nonzero; ftmi_embed_bank; ftmi_l1_loss,
 * ftmi_cross_entropy, ftmi_mol_loss and their *_workspace_bytes; ftmi_run_chain;
 * 21: ftmi_gemm_route, ftmi_conv1d_route, ftmi_conv_bank_route, ftmi_highway_route,
 * ftmi_gemm_switches_digest; no existing signature changed;
 * 22: ftmi_rnn_route, ftmi_rnn_switches_digest; no existing signature changed;
 * added under 22 without a signature change: ftmi_frame_power, ftmi_trim_bounds, ftmi_peak_abs,
 * ftmi_prepare_audio; ftmi_wavernn_packed, ftmi_wr_unfold_packed; ftmi_wavernn_route,
 * ftmi_wr_check_folds, ftmi_wr_check_items; ftmi_fill_tail, ftmi_maxpool_rows,
 * ftmi_duration_counts_rows). */
int ftmi_abi_version(void);
/* sha256 (hex) of the sources this library was built from (the .hip and .h files of
 * forwardtacotron_amd/csrc and include/ftmi.h): the Python binding refuses a library whose
 * id differs from the sources next to it (a stale prebuilt binary). */
const char *ftmi_build_id(void);
/* Static string for an error code (FTMI_E_* or hipError_t). */
const char *ftmi_strerror(int code);
/* Persistent kernels (ftmi_rnn_bidir, ftmi_highway_stack_spread, ftmi_wavernn,
 * ftmi_tacotron_decoder) hold every
 * workgroup of their grid resident while they wait on each other: each checks, before it
 * launches anything, that the kernel's occupancy times the CU count covers its grid, and
 * returns FTMI_E_UNSUPPORTED otherwise (ABI 19).  This sets the CU count the check assumes
 * (0 = the device's; a test hook for the refusal path); returns the previous setting. */
int32_t ftmi_set_resident_cu_limit(int32_t cus);

/* ------------------------------------------------------------------------------------
 * Embedding gather.  out[n, :] = table[ids[n], :]
 * Replaces nn.Embedding forward: models/forward_tacotron.py:125,304 and the predictor
 * embeddings :31,47.  Ids outside [0, num_rows) produce a zero row and set *err = 1
 * (the reference raises IndexError); err may be NULL.
 * ---------------------------------------------------------------------------------- */
int ftmi_embedding(const int64_t *ids, int64_t n, const float *table, int64_t num_rows,
                   int64_t dim, float *out, int32_t *err, ftmi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Fused Conv1d (implicit GEMM on fp32 MFMA) over channels-last sequences.
 *   acc[b,t,n] = sum_{j<k} sum_c w[n, j*Cin + c] * xin[b, t + j - pad, c]   (zero outside [0,T))
 *   for t in [0, T_out)
 *   v = acc (+ bias[n]) ; relu? max(v,0) ; bn? v*bn_scale[n] + bn_shift[n] ; (+ residual)
 *   xin[b,t,:] = x[b,t,:]                              if maxpool == 0
 *              = max(x[b,t-1,:], x[b,t,:]) (t>0), x[b,0,:] (t==0)   if maxpool == 1
 * Replaces BatchNormConv (models/forward_tacotron.py:58-71, models/common_layers.py:38-52),
 * the CBHG maxpool+projections+residual (common_layers.py:100-109), nn.Linear layers
 * (k = 1: pre_highway :113, lin / post_proj forward_tacotron.py:322,326, RNN input
 * projections).  w is packed [N][k*Cin] (tap-major K).  Requires Cin % 16 == 0 and
 * 16-byte aligned x / w / y with strides % 4 == 0.  yt (optional) receives the same
 * values transposed to (B, N, T) — the reference's mel layout.
 * ---------------------------------------------------------------------------------- */
typedef struct ftmi_conv_args {
  const float *x;
  int64_t x_stride; /* floats between consecutive (b,t) rows of x */
  int32_t B, T, Cin;
  const float *w; /* [N][k*Cin] */
  int32_t N, k, pad;
  const float *bias;     /* [N] or NULL */
  int32_t relu;          /* 0 / 1 */
  const float *bn_scale; /* [N] or NULL (BN eval folded: gamma / sqrt(var + eps)) */
  const float *bn_shift; /* [N] (beta - mean * scale) */
  int32_t maxpool;       /* 0 / 1 */
  const float *residual; /* (B,T,N) rows with res_stride, or NULL */
  int64_t res_stride;
  float *y; /* (B,T,N) rows with y_stride, or NULL if only yt is wanted */
  int64_t y_stride;
  float *yt; /* (B,N,T_out) or NULL */
  int32_t T_out; /* output frames per sequence, 0 = T (even k in PyTorch gives T+1) */
  int32_t mma;   /* matrix path: FTMI_MMA_F32, FTMI_MMA_BF16X6 or FTMI_MMA_F16X3 */
  int32_t split_k;  /* > 1: split K over that many workgroups (FTMI_MMA_BF16X6 / F16X3);
                       partial sums go to split_ws and a second launch sums them in fixed
                       order (deterministic) and applies the epilogue */
  float *split_ws;  /* split_k * B*T_out * N floats of caller-owned workspace, or NULL */
  const void *w_split; /* FTMI_MMA_BF16X6: optional ftmi_split_weights pieces (skips the
                          per-call weight split); FTMI_MMA_F16X3: REQUIRED
                          ftmi_split_weights_f16 planes */
  uint32_t *status;    /* optional device word: bit 0 set on f16 range overflow (F16X3) */
  int32_t x_split;     /* ABI 10: x holds f16x3 SPLIT ROWS (below) instead of floats; only
                          FTMI_MMA_F16X3 without maxpool on the slab kernel (B*T_out > 256
                          rows), else FTMI_E_UNSUPPORTED.  x_stride (floats) >= Cin. */
} ftmi_conv_args;

/* f16x3 split rows (ABI 10): the activation layout one f16x3 GEMM hands the next.  Row r
 * of a (rows, C) operand with row stride S floats holds, as halves, C heads h = f16(v) then
 * C scaled tails t = f16((v - h) * 2^11) (v = h + 2^-11 t to ~2^-22 relative): the same 4
 * bytes per element as fp32, the split done once by the producer instead of by every
 * column tile of every consumer, which also checks the f16 range (status bit 0). */

/* Split fp32 weights [N][K] once into three bf16 pieces (w = p0 + p1 + p2 exactly), laid
 * out [3][N][Kpad], Kpad = roundup(K, 32), zero padded; out must hold
 * ftmi_split_weights_bytes(N, K) bytes (16-byte aligned). */
int64_t ftmi_split_weights_bytes(int64_t N, int64_t K);
int ftmi_split_weights(const float *w, int64_t N, int64_t K, void *out, ftmi_stream_t stream);

/* Split fp32 weights [N][K] once for FTMI_MMA_F16X3: per row n a power-of-two scale
 * s_n = 2^-e that normalises the row (8 <= max|w[n]| s_n < 16, e >= -100, which also
 * scales small rows up into the normal f16 range; an all-zero row: e = 0), h = f16(w s_n),
 * t = f16((w s_n - h) * 2^11); layout: f16 planes [3][N][Kpad] = (2^11 h, t, h), Kpad =
 * roundup(K, 32), zero padded, then float colscale[N] = 2^-11 / s_n.  out must hold
 * ftmi_split_weights_f16_bytes(N, K) bytes (16-byte aligned).  The conv bank's w_split
 * is each group's block back to back. */
int64_t ftmi_split_weights_f16_bytes(int64_t N, int64_t K);
int ftmi_split_weights_f16(const float *w, int64_t N, int64_t K, void *out,
                           ftmi_stream_t stream);

int ftmi_conv1d(const ftmi_conv_args *args, ftmi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * CBHG convolution bank: K BatchNormConvs with kernel sizes 1..K (pad k//2, ReLU then
 * BN, output sliced to T), concatenated on channels (common_layers.py:67-71,92-97).
 *   y[b,t, g*Cout + n] = BN_g(relu(sum_{j<=g} sum_c w_g[n, j*Cin+c] * x[b, t+j-(g+1)/2, c]))
 * w: the K packed weights back to back, group g is [Cout][(g+1)*Cin] starting at float
 * offset Cout*Cin*g*(g+1)/2.  bn_scale / bn_shift: [K*Cout].  y: (B,T,K*Cout) rows.
 * w_split: each group's ftmi_split_weights (BF16X6, optional) or ftmi_split_weights_f16
 * (F16X3, required) block back to back.  status: as in ftmi_conv_args.
 * ---------------------------------------------------------------------------------- */
int ftmi_conv_bank(const float *x, int64_t x_stride, int32_t B, int32_t T, int32_t Cin,
                   const float *w, const void *w_split, int32_t K, int32_t Cout,
                   const float *bn_scale,
                   const float *bn_shift, float *y, int64_t y_stride, int32_t mma,
                   uint32_t *status, ftmi_stream_t stream);

/* ftmi_conv_bank with a channel split (ABI 6): when B*T <= 256 and mma == FTMI_MMA_F16X3
 * the bank runs on the weight-streaming "skinny" kernel (B = 1 generation, BASELINE config
 * c2), whose blocks take ceil(ceil(Cin/32) / split_k) <= 2 channel chunks each and leave
 * raw partial sums in split_ws (split_k * B*T * K*Cout floats, caller-owned), summed in split
 * order by a finishing launch (deterministic).  split_k <= 1 / split_ws NULL: as
 * ftmi_conv_bank.  Other shapes ignore the split.  ftmi_conv1d takes the same kernel for
 * B*T_out <= 256 (its split_k / split_ws as documented there).
 * pool_out (ABI 9, flags since ABI 10): FTMI_BANK_POOL — y receives the CBHG maxpool(2, 1)
 * of the bank output (common_layers.py:73,100: y[t] = max(bank[t - 1], bank[t]) within each
 * sequence, y[0] = bank[0]) — the input proj1 then reads with ftmi_conv_args.maxpool = 0;
 * only on the f16x3 slab kernel (mma = FTMI_MMA_F16X3, B*T > 256 rows, no split), elsewhere
 * FTMI_E_UNSUPPORTED.  | FTMI_BANK_Y_SPLIT: y as split rows (proj1 then reads them with
 * ftmi_conv_args.x_split = 1).  FTMI_BANK_X_SPLIT: x is given as split rows. */
/* Floats of the FTMI_BANK_HALVES workspace (counters included) for a bank of B*T <= 128
 * rows, K groups of Cout columns; 0 for other sizes. */
int64_t ftmi_conv_bank_halves_ws_floats(int32_t B, int32_t T, int32_t K, int32_t Cout);
/* Bytes of the FTMI_BANK_IMAGE weight image of a bank (Cin input channels, K groups of Cout
 * columns; any B*T); 0 for shapes FTMI_BANK_HALVES refuses. */
int64_t ftmi_conv_bank_halves_image_bytes(int32_t Cin, int32_t K, int32_t Cout);
/* Builds that image (16-B aligned, ftmi_conv_bank_halves_image_bytes bytes) from the bank's
 * f16x3 split blocks (the FTMI_MMA_F16X3 w_split of ftmi_conv_bank_split); stream-ordered.
 * Once per weights version: it replaces `w_split` (a prepared layout like the split blocks
 * themselves, models/common_layers.py:68-71's bank weights reordered, not recomputed). */
int ftmi_conv_bank_halves_image(const void *w_split, int32_t Cin, int32_t K, int32_t Cout,
                                void *image, ftmi_stream_t stream);
int ftmi_conv_bank_split(const float *x, int64_t x_stride, int32_t B, int32_t T, int32_t Cin,
                         const float *w, const void *w_split, int32_t K, int32_t Cout,
                         const float *bn_scale, const float *bn_shift, float *y,
                         int64_t y_stride, int32_t mma, uint32_t *status, int32_t split_k,
                         float *split_ws, int32_t pool_out, ftmi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Conv bank of an EMBEDDED sequence as a table gather (added under ABI 20): the bank of
 * kernel sizes kmin..kmax (pad k/2, ReLU then BN, as ftmi_conv_bank) applied to
 * embedding(ids) — the prenet CBHG bank (models/forward_tacotron.py:304-306 feeds it the
 * embedding; kmin = 1) and a SeriesPredictor's first conv (:31-36,47-49; kmin = kmax = 5).
 * A convolution of embedding rows is linear in them, so W_k[:, :, j] . E[s] is a constant of
 * the weights:
 *   table [num_rows][taps][Cout] fp32, taps ordered (k = kmin..kmax, j = 0..k-1), holds it;
 *   y[b, t, (k - kmin) Cout + n] = BN_k(relu(sum_{j < k, 0 <= t + j - k/2 < T}
 *                                            table[ids[b, t + j - k/2]][(k, j)][n]))
 * summed in tap order in fp32: bit-identical from launch to launch.  Taps outside their own
 * sequence add nothing; an id outside [0, num_rows) contributes zero (ftmi_embedding's zero
 * row; reporting it stays that call's job).  bn_scale / bn_shift: [G * Cout], G = kmax - kmin
 * + 1.  y: (B, T, G * Cout) rows with y_stride floats.  flags: FTMI_BANK_POOL — y receives the
 * CBHG maxpool(2, 1) of that (y[t] = max(bank[t - 1], bank[t]), y[0] = bank[0]);
 * FTMI_BANK_Y_SPLIT — y as f16x3 split rows of G * Cout (the operand of
 * ftmi_conv_args.x_split), a value beyond 65504 in magnitude or not a number sets status
 * bit 0 (optional word).
 * kmax <= 16 and Cout % 256 == 0, else FTMI_E_UNSUPPORTED; table / bn / y 16-B aligned.
 * ---------------------------------------------------------------------------------- */
int ftmi_embed_bank(const int64_t *ids, int32_t B, int32_t T, const float *table,
                    int32_t num_rows, int32_t kmin, int32_t kmax, int32_t Cout,
                    const float *bn_scale, const float *bn_shift, float *y, int64_t y_stride,
                    int32_t flags, uint32_t *status, ftmi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * One highway layer (common_layers.py:22-35):
 *   g = sigmoid(x W2^T + b2);  y = g * relu(x W1^T + b1) + (1 - g) * x
 * w12: [2C][C] with rows interleaved in blocks of 32: rows 64q..64q+31 = W1 rows
 * 32q..32q+31, rows 64q+32..64q+63 = W2 rows 32q..32q+31.  Requires C % 32 == 0.
 * w12_split: ftmi_split_weights (BF16X6, optional) / ftmi_split_weights_f16 (F16X3,
 * required) of w12.  status: as in ftmi_conv_args.  y must not alias x.
 * ---------------------------------------------------------------------------------- */
int ftmi_highway(const float *x, int64_t x_stride, int64_t M, int32_t C, const float *w12,
                 const void *w12_split, const float *b1, const float *b2, float *y,
                 int64_t y_stride, int32_t mma, uint32_t *status, ftmi_stream_t stream);

/* ftmi_highway with a channel split (ABI 6): split_k >= 1 with M <= 1024 rows and
 * mma == FTMI_MMA_F16X3 runs the weight-streaming skinny kernel, whose blocks leave raw
 * partial sums of x [W1|W2]^T in split_ws (split_k * M * 2C floats, caller-owned) and a
 * finishing launch sums them in split order and applies the gating (deterministic).
 * split_k = 0 / other shapes: as ftmi_highway. */
int ftmi_highway_split(const float *x, int64_t x_stride, int64_t M, int32_t C,
                       const float *w12, const void *w12_split, const float *b1,
                       const float *b2, float *y, int64_t y_stride, int32_t mma,
                       uint32_t *status, int32_t split_k, float *split_ws,
                       ftmi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Which kernel a conv / bank / highway launch takes (ABI 21).  The library decides it in one
 * function, from the launch's arguments and the routing switches it reads from the
 * environment on every call (FTMI_GEMM_SLAB, FTMI_GEMM_SLAB_MIN, FTMI_GEMM_SLAB_WS,
 * FTMI_SLAB_K1_NMIN, FTMI_SLAB_PF, FTMI_SLAB_BAND, FTMI_GEMM_SKINNY, FTMI_SKINNY_CPB,
 * FTMI_BANK_BALANCED, FTMI_BANK_WALK, FTMI_BANK_HALVES).  The queries below run that function
 * for a caller that has to size a workspace before it launches: host only, no launch, no
 * device call, no pointer dereferenced.  Each takes the arguments of its entry point (so the
 * alignment and stride tests see the real pointers), returns that entry point's argument
 * errors, and otherwise fills *route and returns FTMI_OK.
 * ---------------------------------------------------------------------------------- */
enum { FTMI_ROUTE_UNSUPPORTED = 0, /* the entry point would return FTMI_E_UNSUPPORTED */
       FTMI_ROUTE_SKINNY, FTMI_ROUTE_SKINNY_BANK, /* weight-streaming few-row kernel / its
                                                     balanced bank schedule */
       FTMI_ROUTE_SLAB, FTMI_ROUTE_SLAB_WS, FTMI_ROUTE_SLAB_PF, /* 256 x 128 slab kernels */
       FTMI_ROUTE_BANK_WALK,   /* pooled bank on at most 96 input channels */
       FTMI_ROUTE_BANK_HALVES, /* the one-launch few-row bank: pass FTMI_BANK_HALVES */
       FTMI_ROUTE_X6B_F16, FTMI_ROUTE_X6B_BF16, FTMI_ROUTE_X6, FTMI_ROUTE_F32 /* 128 x 128 tiles */ };
typedef struct ftmi_gemm_route {
  int32_t kernel;    /* FTMI_ROUTE_* */
  int32_t split_k;   /* the split the kernel requires, to be passed with split_ws; 0: none
                        required — the kernel takes whatever split_k its caller chooses (with
                        split_k * rows * N floats) or none */
  int64_t ws_floats; /* floats of split_ws for that split_k (FTMI_ROUTE_BANK_HALVES: the
                        counters included, as ftmi_conv_bank_halves_ws_floats) */
  int32_t pooled;    /* the FTMI_BANK_POOL / FTMI_BANK_Y_SPLIT store asked for is accepted */
  int32_t band;      /* slab kernels: the column-band tile order (FTMI_SLAB_BAND), else 0 */
} ftmi_gemm_route;
/* args->split_k / split_ws are ignored. */
int ftmi_conv1d_route(const ftmi_conv_args *args, ftmi_gemm_route *route);
/* flags: FTMI_BANK_POOL | FTMI_BANK_Y_SPLIT | FTMI_BANK_X_SPLIT only. */
int ftmi_conv_bank_route(const float *x, int64_t x_stride, int32_t B, int32_t T, int32_t Cin,
                         const float *w, const void *w_split, int32_t K, int32_t Cout,
                         const float *bn_scale, const float *bn_shift, float *y,
                         int64_t y_stride, int32_t mma, uint32_t *status, int32_t flags,
                         ftmi_gemm_route *route);
int ftmi_highway_route(const float *x, int64_t x_stride, int64_t M, int32_t C,
                       const float *w12, const void *w12_split, const float *b1,
                       const float *b2, float *y, int64_t y_stride, int32_t mma,
                       uint32_t *status, ftmi_gemm_route *route);
/* 64-bit digest of the routing switches as the next launch would read them: equal digests,
 * equal routes for equal arguments (a cached launch list is keyed by it). */
uint64_t ftmi_gemm_switches_digest(void);

/* CBHG highway stack in one launch (ABI 9; common_layers.py:110-115 + the GRU's input
 * projection): h = x W_pre^T (pre_highway, no bias), then L highway layers as ftmi_highway,
 * then y = h W_out^T + b_out.  Activations stay on chip between layers; the result is
 * bit-identical to the unfused ftmi_conv1d / ftmi_highway chain on FTMI_MMA_F16X3.
 *   x: M rows of Cp floats (Cp % 4 == 0, Cp <= C), C == 256 (the CBHG channels)
 * Every weight operand is an ftmi_split_weights_f16_FRAG block (fragment-major planes):
 *   w_pre_split: of W_pre [C][Cp]
 *   w_hw_split[l], b1[l], b2[l]: host arrays of L (<= 8) device pointers — the block of
 *     each highway's packed w12 [2C][C] and its biases
 *   w_out_split: of W_out [n_out][C] (n_out % 512 == 0) and b_out
 *     (nullable) -> y (M x n_out, row stride y_stride); NULL with n_out = 0, y = NULL: none
 *   h: optional (nullable) copy of the last highway's output (M x C, row stride h_stride)
 * status: bit 0 when an activation is beyond the f16 range (rerun on the unfused exact path).
 * ---------------------------------------------------------------------------------- */
/* ftmi_split_weights_f16 with the planes in the fragment-major order of the 16x16x32 f16
 * MFMA B operand, [N/16][Kpad/32][64][8] (lane = n % 16 + 16 ((k / 8) % 4), element k % 8;
 * ABI 9): same byte size (ftmi_split_weights_f16_bytes), N % 16 == 0. */
int ftmi_split_weights_f16_frag(const float *w, int64_t N, int64_t K, void *out,
                                ftmi_stream_t stream);

/* fp32 rows (rows, C) -> f16x3 split rows (ABI 10; the operand of ftmi_conv_args.x_split /
 * FTMI_BANK_X_SPLIT) for an activation that is also needed in fp32 (a CBHG input is its
 * residual too).  Sets status bit 0 (optional word) if |x| > 65504.  C % 4 == 0, strides in
 * floats >= C, 16-B aligned, y must not alias x. */
int ftmi_split_rows(const float *x, int64_t x_stride, int64_t rows, int32_t C, float *y,
                    int64_t y_stride, uint32_t *status, ftmi_stream_t stream);

int ftmi_highway_stack(const float *x, int64_t x_stride, int64_t M, int32_t Cp, int32_t C,
                       const void *w_pre_split, int32_t L, const void *const *w_hw_split,
                       const float *const *b1, const float *const *b2,
                       const void *w_out_split, const float *b_out, int32_t n_out, float *y,
                       int64_t y_stride, float *h, int64_t h_stride, uint32_t *status,
                       ftmi_stream_t stream);

/* The same CBHG tail for few rows (ABI 18; batch-1 generation, BASELINE config c2: the
 * prenet's 120 and the postnet's 816 rows), spread over the chip: each 64-row block over 16
 * workgroups that own 16 channels of every layer (and n_out / 16 output columns) and exchange
 * the layers' activations through `ws` — bit-identical to ftmi_highway_stack.  M <= 1024,
 * n_out <= 1536, and the ftmi_highway_stack_spread_blocks(M) workgroups must all be resident
 * at once (<= the CU count; they wait on each other: run it where no other persistent kernel
 * holds the CUs it needs), else FTMI_E_UNSUPPORTED.  ws: 16-B aligned device workspace of
 * ftmi_highway_stack_spread_ws_bytes(M) bytes, one per stream (its counters are zeroed by
 * the call).  A workgroup that waits past its spin bound sets FTMI_STATUS_RNN_TIMEOUT.
 * Replaces common_layers.py:110-118 (pre_highway, highways, the GRU's input GEMM). */
int64_t ftmi_highway_stack_spread_ws_bytes(int64_t M);
int32_t ftmi_highway_stack_spread_blocks(int64_t M);
int ftmi_highway_stack_spread(const float *x, int64_t x_stride, int64_t M, int32_t Cp,
                              int32_t C, const void *w_pre_split, int32_t L,
                              const void *const *w_hw_split, const float *const *b1,
                              const float *const *b2, const void *w_out_split,
                              const float *b_out, int32_t n_out, float *y, int64_t y_stride,
                              float *h, int64_t h_stride, uint32_t *status, void *ws,
                              ftmi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Bidirectional single-layer GRU / LSTM recurrence, PyTorch semantics, h0 = c0 = 0,
 * both directions over the full padded length (no packing), output [fwd | bwd].
 *   GRU  (cell = 0, gates r,z,n): common_layers.py:84,118 and forward_tacotron.py:39,53
 *   LSTM (cell = 1, gates i,f,g,o): forward_tacotron.py:165-168,321
 * xp: precomputed input projections, rows of 2*G*H floats ([dir][gate][unit]), already
 *     including b_ih (GRU) or b_ih + b_hh (LSTM); row for (b, t) is
 *       xp + (b*T_src + src)*xp_stride,  src = t if index == NULL else index[b*T + t];
 *     src < 0 selects xp_zero (the projection of a zero input row: the biases), 2*G*H.
 *     (index = LengthRegulator map: the LSTM reads phoneme-rate projections directly.)
 * w_hh: [2][G*H][H] (PyTorch weight_hh_l0 then weight_hh_l0_reverse).
 * b_hh: [2][G*H] for GRU (added inside the recurrence), ignored (may be NULL) for LSTM.
 * lengths: int32 [B] or NULL.  Packed-sequence semantics (pack_padded_sequence +
 *     pad_packed_sequence, forward_tacotron.py:224-230): frames t >= lengths[b] output
 *     pad_value and the reverse direction starts from h = c = 0 at t = lengths[b]-1.
 * y:    (B, T, 2H) rows with y_stride.
 * mma:  matrix path of W_hh h: FTMI_MMA_F16X3 (default; W_hh split in-kernel, bit 1 of
 *     *status set if an entry exceeds the f16 range — rerun with FTMI_MMA_BF16X6),
 *     FTMI_MMA_BF16X6 or FTMI_MMA_F32.  status: optional device word.  ABI 12: OR
 *     FTMI_RNN_SPREAD into mma to let the call spread a small-H recurrence over the whole
 *     device (fewer sequences per workgroup group: lower step latency, more workgroups —
 *     for a recurrence that runs alone; ftmi_rnn_blocks takes the same flag).
 * sync: 16-byte aligned device workspace of ftmi_rnn_workspace_bytes() bytes (zeroed by
 *     the call; holds the arrival counters and the h exchange buffer).  After the stream
 *     has completed, the 32-bit word at byte offset ftmi_rnn_error_offset() is non-zero if
 *     a workgroup timed out waiting for its group (not all workgroups resident); the same
 *     event sets FTMI_STATUS_RNN_TIMEOUT in *status.
 * Supported H: GRU 64, 128, 256; LSTM 512 (the ForwardTacotron config).
 * ---------------------------------------------------------------------------------- */
enum { FTMI_RNN_SPREAD = 0x100 };
int64_t ftmi_rnn_workspace_bytes(int32_t B, int32_t H, int32_t cell);
int64_t ftmi_rnn_error_offset(int32_t B);
/* Workgroups the (first) launch of ftmi_rnn_bidir(cell, B, H, mma) occupies: each is
 * persistent (one per CU) and waits on the others, so recurrences issued concurrently on
 * several streams must not exceed the CU count together (the host serialises them
 * otherwise).  0 for an unsupported shape. */
int32_t ftmi_rnn_blocks(int32_t cell, int32_t B, int32_t H, int32_t mma);
/* ABI 22: everything ftmi_rnn_bidir(cell, B, ., H, ..., mma) decides before it launches, from
 * one host function that reads its switches in the environment on every call (FTMI_RNN_GEMV,
 * FTMI_RNN_GEMV_KSEG, FTMI_RNN_XCD_LOCAL, FTMI_RNN_PAD, FTMI_RNN_U64, FTMI_RNN_CSTORE,
 * FTMI_RNN_CELLROWS, FTMI_RNN_NB, FTMI_RNN_U8, FTMI_RNN_PSLEEP).  ftmi_rnn_route runs it
 * without a launch, a device write or a pointer; ftmi_rnn_blocks is its first_blocks (0 when
 * status is not FTMI_OK).  mma may carry FTMI_RNN_SPREAD; cus: the CUs to plan for, 0 = the
 * current device's.  FTMI_E_ARG for a NULL out, B or H <= 0, cus < 0, or an mma that
 * ftmi_rnn_bidir refuses. */
enum { FTMI_RNN_KERNEL_NONE = 0, FTMI_RNN_KERNEL_GEMV, /* rnn_gemv_kernel<cell, H, units, nbv, kseg> */
       FTMI_RNN_KERNEL_BIDIR /* rnn_bidir_kernel<cell, H, units, wk, mode, cst, nbl, cr> */ };
typedef struct ftmi_rnn_route {
  int32_t status;          /* FTMI_OK, or FTMI_E_UNSUPPORTED as ftmi_rnn_bidir would return */
  int32_t kernel;          /* FTMI_RNN_KERNEL_* */
  int32_t cell;
  int32_t H;
  int32_t units;           /* hidden units per workgroup */
  int32_t wk;              /* BIDIR: K-split waves */
  int32_t mode;            /* BIDIR: the matrix path (FTMI_MMA_*) */
  int32_t cst;             /* BIDIR: the compute waves store h */
  int32_t nbl;             /* BIDIR: live sequences per group */
  int32_t cr;              /* BIDIR: cell-row W_hh order */
  int32_t kseg;            /* GEMV: k-segments per row */
  int32_t nbv;             /* GEMV: sequences per workgroup */
  int32_t threads;         /* per workgroup */
  int32_t wg_per_group;    /* workgroups that exchange h each step: H / units */
  int32_t groups;          /* over all passes: two directions per chunk of sequences */
  int32_t groups_per_pass; /* most groups one launch holds on `cus` CUs */
  int32_t passes;          /* launches */
  int32_t first_blocks;    /* workgroups of the first launch, padding included */
  int32_t xcd_local;       /* FTMI_RNN_XCD_LOCAL as the kernel receives it */
  int32_t pad;             /* fewer than 8 groups are padded to one per XCD (if xcd_local) */
  int32_t psleep;          /* s_sleep(1) count before a step's first h poll */
  int32_t cus;             /* the CU count the grid was planned for */
} ftmi_rnn_route_t;
int ftmi_rnn_route(int32_t cell, int32_t B, int32_t H, int32_t mma, int32_t cus,
                   ftmi_rnn_route_t *out);
/* 64-bit digest of those switches as the next call would read them: equal digests, equal
 * routes for equal arguments. */
uint64_t ftmi_rnn_switches_digest(void);
/* Test / diagnostic hook: bound of every recurrence spin (polls per wait) for launches
 * issued after the call; 0 restores the default (2^22).  Returns the previous bound. */
uint32_t ftmi_set_rnn_spin_limit(uint32_t limit);
int ftmi_rnn_bidir(int32_t cell, int32_t B, int32_t T, int32_t H, const float *xp,
                   int64_t xp_stride, int32_t T_src, const int32_t *index,
                   const float *xp_zero, const float *w_hh, const float *b_hh,
                   const int32_t *lengths, float pad_value, float *y, int64_t y_stride,
                   int32_t mma, uint32_t *status, void *sync, ftmi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Duration post-processing of ForwardTacotron.generate + LengthRegulator counts:
 *   if sum_{b,t} trunc_int64(dur) <= 0: dur[:] = fill_value   (forward_tacotron.py:254-255,
 *                                                               only when apply_fill != 0)
 *   dur[dur < 0] = 0                    (in place, common_layers.py:13)
 *   count = int64(trunc(fp32(dur + 0.5)))  (common_layers.py:16)
 *   offsets[b, 0..T] = exclusive prefix sum of counts; totals[b] = offsets[b, T]
 * Single launch, bit-exact. offsets: int32 [B][T+1]; totals: int32 [B];
 * fill_flag (optional int32[1]) receives 1 if the fill rule fired.
 * ---------------------------------------------------------------------------------- */
int ftmi_duration_counts(float *dur, int32_t B, int32_t T, int32_t apply_fill,
                         float fill_value, int32_t *offsets, int32_t *totals,
                         int32_t *fill_flag, ftmi_stream_t stream);

/* Batch-sharded form of the fill-2 rule: the reference decides on the sum
 * over the WHOLE batch, so each shard computes its partial sum (ftmi_duration_trunc_sum:
 * out[0] = sum_{b,t} trunc_int64(dur)), the host all-reduces it (RCCL SUM, device int64),
 * and ftmi_duration_counts_global applies the rule with that global sum, then clips /
 * counts / scans exactly like ftmi_duration_counts. */
int ftmi_duration_trunc_sum(const float *dur, int32_t B, int32_t T, int64_t *out,
                            ftmi_stream_t stream);
int ftmi_duration_counts_global(float *dur, int32_t B, int32_t T, const int64_t *global_sum,
                                float fill_value, int32_t *offsets, int32_t *totals,
                                int32_t *fill_flag, ftmi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Length-aware batches (ForwardTacotron.generate_masked): item b of a padded batch holds
 * len[b] valid rows from row 0 on; these restore at its right edge what the item run alone
 * would see.  len / x_len: device int32 [B]; a negative entry counts as 0.
 *
 * ftmi_fill_tail writes `value` to rows [len[b], min(T, len[b] + reach)) of every item
 * (reach < 0: up to T; reach == 0 or len[b] >= T: nothing).  It never writes at or past row
 * T of an item and never between C and the stride.  mode:
 *   FTMI_FILL_ROWS        x is (B, T, C) fp32 rows, `stride` floats per row (>= C), item
 *                         stride T * stride.  16-byte stores when C % 4 == 0, stride % 4 == 0
 *                         and x is 16-byte aligned, 4-byte stores otherwise.
 *   FTMI_FILL_TIME_LAST   x is (B, C, T), `stride` floats per channel (>= T), item stride
 *                         C * stride; 4-byte stores.
 *   FTMI_FILL_SPLIT_ROWS  as FTMI_FILL_ROWS, the rows holding f16x3 split rows (above): C
 *                         heads f16(value), then C tails f16((value - h) 2^11); C % 2 == 0
 *                         (else FTMI_E_SHAPE), 16-byte stores when C % 8 == 0.  value = 0 is
 *                         all-zero halves.
 * A stride below C (T for FTMI_FILL_TIME_LAST): FTMI_E_SHAPE; an unknown mode: FTMI_E_ARG.
 *
 * ftmi_maxpool_rows is the CBHG maxpool (MaxPool1d(2, 1, padding=1)[..., :T]) of (B, T, C)
 * rows with such ends: y[b,t] = max(x[b,t-1], x[b,t]) (t = 0: x[b,0]) for t < len[b], zero
 * rows from len[b] on.  C % 4 == 0, strides % 4 == 0, x / y 16-byte aligned (FTMI_E_ALIGN).
 *
 * ftmi_duration_counts_rows is ftmi_duration_counts decided per item: positions
 * t >= x_len[b] get duration 0 and count 0 (x_len[b] > T counts as T); with apply_fill,
 * row b is filled where sum_{t < x_len[b]} trunc_int64(dur[b,t]) <= 0, at its valid
 * positions only; the clip, the count and the scan are the same arithmetic, bit for bit.
 * fill_flags (optional int32 [B]) receives 1 for every row the rule filled.
 * ---------------------------------------------------------------------------------- */
enum { FTMI_FILL_ROWS = 0, FTMI_FILL_TIME_LAST = 1, FTMI_FILL_SPLIT_ROWS = 2 };
int ftmi_fill_tail(float *x, int64_t stride, int32_t B, int32_t T, int32_t C,
                   const int32_t *len, int32_t reach, float value, int32_t mode,
                   ftmi_stream_t stream);
int ftmi_maxpool_rows(const float *x, int64_t x_stride, int32_t B, int32_t T, int32_t C,
                      const int32_t *len, float *y, int64_t y_stride, ftmi_stream_t stream);
int ftmi_duration_counts_rows(float *dur, int32_t B, int32_t T, const int32_t *x_len,
                              int32_t apply_fill, float fill_value, int32_t *offsets,
                              int32_t *totals, int32_t *fill_flags, ftmi_stream_t stream);

/* Frame -> phoneme index map of the LengthRegulator: index[b, f] = t such that
 * offsets[b,t] <= f < offsets[b,t+1], or -1 for f >= totals[b] (zero padding,
 * pad_sequence in common_layers.py:18).  index: int32 [B][T_mel]; T_mel = 0 launches nothing
 * and takes a null index (an empty map has no storage). */
int ftmi_lr_index(const int32_t *offsets, int32_t B, int32_t T, int32_t T_mel,
                  int32_t *index, ftmi_stream_t stream);

/* LengthRegulator expansion (common_layers.py:12-19): y[b,f,:] = x[b,index[b,f],:] or 0. */
int ftmi_length_regulate(const float *x, int64_t x_stride, int32_t B, int32_t T, int32_t C,
                         const int32_t *index, int32_t T_mel, float *y, int64_t y_stride,
                         ftmi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Pitch / energy conditioning (forward_tacotron.py:308-314):
 *   x[b,t,c] = (x[b,t,c] + P[b,t,c] * pitch_strength) + E[b,t,c] * energy_strength
 *   P = Conv1d(1 -> C, k=3, pad=1, bias)(pitch[b,:]) at t (same for E with energy).
 * pitch / energy: (B, T) contiguous. wp / we: [C][3]; bp / be: [C].
 * ---------------------------------------------------------------------------------- */
int ftmi_series_proj_add(float *x, int64_t x_stride, int32_t B, int32_t T, int32_t C,
                         const float *pitch, const float *wp, const float *bp,
                         float pitch_strength, const float *energy, const float *we,
                         const float *be, float energy_strength, ftmi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * SeriesPredictor head (forward_tacotron.py:41,54-55): out[m] = (x[m,:] . w + bias[0]) / alpha
 * x: M rows of C floats (row stride x_stride); bias: device float[1] or NULL; out: M floats.
 * ---------------------------------------------------------------------------------- */
int ftmi_rowdot(const float *x, int64_t x_stride, int64_t M, int32_t C, const float *w,
                const float *bias, float alpha, float *out, ftmi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Launch lists (added under ABI 20): a chain of the launches above issued by ONE call, so
 * the host pays one foreign call per chain instead of one per kernel.  The caller builds the
 * list once per shape and reuses it from call to call with only the bases patched.
 *
 * An op is a tagged record.  Every pointer argument is a reference into a base table:
 * (slot, byte offset, byte extent); slot < 0 is a NULL pointer.  The extent is the range the
 * op may touch from that pointer on; FTMI_CHAIN_ALIGN16 demands a 16-byte aligned address.
 * The integer / float arguments of the entry point travel in i[] / f[] in the order below
 * (the entry point's own argument order, pointers left out):
 *   FTMI_CHAIN_EMBEDDING  p: ids, table, out, err          i: n, num_rows, dim
 *   FTMI_CHAIN_CONV1D     p: x, w, bias, bn_scale, bn_shift, residual, y, yt, split_ws,
 *                            w_split, status
 *                         i: x_stride, B, T, Cin, N, k, pad, relu, maxpool, res_stride,
 *                            y_stride, T_out, mma, split_k, x_split
 *   FTMI_CHAIN_RNN_BIDIR  p: xp, index, xp_zero, w_hh, b_hh, lengths, y, status, sync
 *                         i: cell, B, T, H, xp_stride, T_src, y_stride, mma   f: pad_value
 *   FTMI_CHAIN_ROWDOT     p: x, w, bias, out               i: x_stride, M, C   f: alpha
 *
 * ftmi_run_chain first validates the whole list and launches nothing unless it passes:
 * n > 0, every tag known, every slot inside the table with a non-NULL base, every
 * [offset, offset + extent) inside its slot's declared size, every flagged address aligned,
 * and every range an op WRITES (conv y / yt / split_ws, recurrence y / sync, embedding out,
 * rowdot out) at least as large as the op's shape needs.  A failure returns
 * FTMI_E_ARG (FTMI_E_ALIGN for alignment) with *failed_op = the offending op (-1: the list
 * itself).  Then the ops run in order through the entry points above on `stream`; the first
 * non-zero return stops the list and is returned with *failed_op = that op's index (earlier
 * ops stay queued).  No synchronisation, no allocation, no state of its own: safe on several
 * streams at once and inside stream capture.  failed_op may be NULL.
 * ---------------------------------------------------------------------------------- */
enum { FTMI_CHAIN_EMBEDDING = 1, FTMI_CHAIN_CONV1D = 2, FTMI_CHAIN_RNN_BIDIR = 3,
       FTMI_CHAIN_ROWDOT = 4 };
enum { FTMI_CHAIN_ALIGN16 = 1 };
enum { FTMI_CHAIN_PTRS = 12, FTMI_CHAIN_INTS = 16, FTMI_CHAIN_FLOATS = 2 };
typedef struct ftmi_chain_ref {
  int32_t slot;  /* index into the base table, < 0: NULL */
  int32_t flags; /* FTMI_CHAIN_ALIGN16 */
  int64_t offset, bytes;
} ftmi_chain_ref;
typedef struct ftmi_chain_op {
  int32_t tag, reserved;
  ftmi_chain_ref p[FTMI_CHAIN_PTRS];
  int64_t i[FTMI_CHAIN_INTS];
  float f[FTMI_CHAIN_FLOATS];
} ftmi_chain_op;
typedef struct ftmi_chain_base {
  void *base;    /* device address of the slot (ids, a packed weight, workspace, output ...) */
  int64_t bytes; /* its declared size */
} ftmi_chain_base;
int ftmi_run_chain(const ftmi_chain_op *ops, int32_t n, const ftmi_chain_base *bases,
                   int32_t n_bases, int32_t *failed_op, ftmi_stream_t stream);

/* ====================================================================================
 * Audio path: utils/dsp.py (DSP.wav_to_mel :71-87, griffinlim :89-103), whose arithmetic
 * is librosa 0.7.2 (requirements.txt:2): core.stft / core.istft / filters.mel /
 * util.nnls / core.griffinlim.  Plans (host-built once per DSP config, device buffers):
 *   window  double[n_fft]     periodic Hann of win_length, zero-padded to n_fft (centred)
 *   win_sq  double[n_fft]     window**2 (window_sumsquare's envelope)
 *   twiddle double[n_fft][2]  exp(-2 pi i k / n_fft), k < n_fft / 2
 * n_fft: power of two in [16, 4096].  center=True, pad_mode='reflect' throughout.
 * Spectra are FRAME-major complex64 (B, F, n_fft/2+1) (interleaved re, im floats); mel
 * is (B, n_mels, F).  `lengths` (samples) / `frames` (frames) are optional device int32
 * per-item limits (NULL: L / F for every item); frames past an item's count are skipped.
 * ==================================================================================== */

/* complex STFT (librosa core.stft: rfft(window * frame) in fp64, stored complex64) of
 * audio rows y (B, L) with row stride y_stride; F = 1 + L // hop frames. */
int ftmi_stft(const float *y, int64_t y_stride, int32_t B, int64_t L, const int32_t *lengths,
              int32_t n_fft, int32_t hop, const double *window, const void *twiddle, int32_t F,
              const int32_t *frames, void *X, ftmi_stream_t stream);

/* DSP.wav_to_mel (utils/dsp.py:71-87): mel[b,i,f] = sum_k basis[i,k] |STFT|[b,f,k]
 * (fp64 accumulation over the row support [mel_lo[i], mel_hi[i]) of basis [n_mels][nb]),
 * then log(max(., 1e-5)) when log_norm (DSP.normalize :105-107). */
int ftmi_mel_spectrogram(const float *y, int64_t y_stride, int32_t B, int64_t L,
                         const int32_t *lengths, int32_t n_fft, int32_t hop, const double *window,
                         const void *twiddle, int32_t F, const int32_t *frames, const float *basis,
                         const int32_t *mel_lo, const int32_t *mel_hi, int32_t n_mels,
                         int32_t log_norm, float *mel, ftmi_stream_t stream);

/* One fast Griffin-Lim analysis step (librosa core.griffinlim loop body): rebuilt =
 * STFT(y); angles = rebuilt - c * tprev (first: rebuilt); angles /= |angles| + 1e-16;
 * X = S * angles (next synthesis input); tprev = rebuilt.  S: (B, F, nb) float32;
 * tprev, X: (B, F, nb) complex64.  c = momentum / (1 + momentum). */
int ftmi_griffinlim_stft(const float *y, int64_t y_stride, int32_t B, int64_t L,
                         const int32_t *lengths, int32_t n_fft, int32_t hop, const double *window,
                         const void *twiddle, int32_t F, const int32_t *frames, const float *S,
                         void *tprev, float c, int32_t first, void *X, ftmi_stream_t stream);

/* X = S * angles elementwise (complex64 = float32 * complex64, numpy rounding): the
 * Griffin-Lim synthesis input for the initial phases.  n = number of bins in total. */
int ftmi_spec_mul(const float *S, const void *angles, int64_t n, void *X, ftmi_stream_t stream);

/* Griffin-Lim's random initial phases (librosa 0.7.2 core.griffinlim:
 * np.exp(2j * np.pi * np.random.rand(n_bins, T))) from the host's uniform draws u (B, n_bins,
 * T) float64, bin-major as numpy draws them: angles (B, T, n_bins) complex64, frame-major
 * (float64 cos / sin, rounded to complex64).  ABI 11. */
int ftmi_unit_phases(const double *u, int32_t B, int32_t n_bins, int32_t T, void *angles,
                     ftmi_stream_t stream);

/* librosa core.istft (center=True): per-frame fp64 irfft * window, overlap-added in frame
 * order with float32 rounding, divided by the window sum-square where > FLT_MIN, cropped
 * by n_fft/2.  Item b yields hop * (frames_b - 1) samples into y[b, :], zero-filled up to
 * y_len.  work: ftmi_istft_workspace_bytes(B, F, n_fft) bytes. */
int64_t ftmi_istft_workspace_bytes(int32_t B, int32_t F, int32_t n_fft);
int ftmi_istft(const void *X, int32_t B, int32_t F, const int32_t *frames, int32_t n_fft,
               int32_t hop, const double *window, const double *win_sq, const void *twiddle,
               void *work, float *y, int64_t y_stride, int64_t y_len, ftmi_stream_t stream);

/* One fast Griffin-Lim iteration in ONE launch (ABI 19; librosa 0.7.2 core.griffinlim loop
 * body, utils/dsp.py:91-102): rebuilt = stft(istft(Xin)); angles = rebuilt - c * tprev
 * (first: rebuilt); angles /= |angles| + 1e-16; Xout = S * angles; tprev = rebuilt — the
 * ISTFT (fp64 irfft, float32 overlap-add in frame order, window sum-square division,
 * center crop) and the STFT (reflect padding) of ftmi_istft / ftmi_griffinlim_stft, fused
 * per tile of 16 frames with the audio kept on chip.  Xin != Xout (neighbouring tiles read
 * Xin's halo frames); spectra (B, F, n_fft/2+1) complex64 frame-major, item b's first
 * frames[b] frames (NULL: F).  n_fft = 1024, hop = 256 only (else FTMI_E_UNSUPPORTED).
 * window / win_sq: [n_fft] float64, twiddle: [n_fft/2] complex128 (the ftmi_stft plan). */
int ftmi_griffinlim_iter(const void *Xin, void *Xout, const float *S, void *tprev, int32_t B,
                         int32_t F, const int32_t *frames, int32_t n_fft, int32_t hop,
                         const double *window, const double *win_sq, const void *twiddle,
                         float c, int32_t first, ftmi_stream_t stream);
/* ftmi_istft in one launch, no workspace (ABI 19; same sizes as ftmi_griffinlim_iter). */
int ftmi_istft_fused(const void *X, int32_t B, int32_t F, const int32_t *frames, int32_t n_fft,
                     int32_t hop, const double *window, const double *win_sq, const void *twiddle,
                     float *y, int64_t y_stride, int64_t y_len, ftmi_stream_t stream);

/* mel -> linear magnitude (librosa feature.inverse.mel_to_stft, power=1, via util.nnls):
 * per frame min ||A x - m||^2, x >= 0, m = exp(mel) when denorm (DSP.denormalize
 * :109-110).  Solved by FISTA (`iters` steps of 1/L = inv_L) from the clipped
 * minimum-norm solution pinv(A) m.  A is given sparse: row i holds nonzeros
 * rowvals[rowptr[i] .. rowptr[i+1]) for bins rowlo[i] ...; bin k feeds mel rows
 * bin_rows[2k], bin_rows[2k+1] (-1: none) with weights bin_w[2k], bin_w[2k+1]; pinv is
 * [n_bins][n_mels].  nnz = rowptr[n_mels].  S: (B, F, n_bins) float32. */
int ftmi_mel_nnls(const float *mel, int32_t B, int32_t F, const int32_t *frames, int32_t n_mels,
                  int32_t n_bins, int32_t denorm, int32_t nnz, const float *rowvals,
                  const int32_t *rowptr, const int32_t *rowlo, const int32_t *bin_rows,
                  const float *bin_w, const float *pinv, float inv_L, int32_t iters, float *S,
                  ftmi_stream_t stream);

/* The reference's NNLS itself (ABI 19): librosa 0.7.2 util.nnls — scipy fmin_l_bfgs_b
 * (L-BFGS-B 3.0, m = n_bins, pgtol 1e-5, factr 1e7, maxls 20) on blocks of up to
 * `max_frames` frames (127 for n_fft 1024: MAX_MEM_BLOCK // (n_bins * 4)), started from the
 * float32 least-squares solution clipped at 0 — so S is the reference's to rounding, not
 * just another minimiser (librosa/util/utils.py nnls, _nnls_lbfgs_block).
 * blocks: device [n_blocks][4] int32 (item, first frame, frames, 0); groups: workgroups per
 * block for the sweeps (1..64); m: history columns the workspace holds (the reference keeps
 * n_bins; a block that needs more stops with bit 4 in status[0]: rerun with a larger m);
 * pinv: [n_bins][n_mels] float64; active: device int32 the caller sets to n_blocks before
 * ftmi_nnls_lbfgsb_start — each block decrements it when done.  Drive it like scipy's
 * driver loop: start, then ftmi_nnls_lbfgsb_cycles (one cycle advances every block by one
 * L-BFGS-B iteration or one extra line-search evaluation) until *active reads 0, then
 * ftmi_nnls_lbfgsb_finish (writes S (B, F, n_bins), zero past frames[b]; status: device
 * int32[2] the caller zeroes: [0] |= failure bits of any block (2 abnormal line search,
 * 4 history full, 8 > 1024 equal breakpoints), [1] = max iterations; info: NULL or device
 * double[n_blocks][4] = per block (iterations, f evaluations, f, projected-gradient norm)). */
typedef struct {
  const float *mel; /* (B, n_mels, F) */
  int32_t B, F, n_mels, n_bins, denorm;
  const int32_t *blocks;
  int32_t n_blocks, groups, m, max_frames;
  int32_t maxiter;   /* scipy's maxiter (0: its default 15000) */
  int32_t dbg_stop;  /* 0; else stop each block before phase (dbg_stop & 15) of iteration dbg_stop >> 4 */
  const float *rowvals;
  const int32_t *rowptr, *rowlo, *bin_rows;
  const float *bin_w;
  const double *pinv;
  void *workspace; /* ftmi_nnls_lbfgsb_workspace_bytes(n_blocks, n_bins, max_frames, m, groups) */
  float *S;
  int32_t *active;
} ftmi_nnls_lbfgsb_args;
int64_t ftmi_nnls_lbfgsb_workspace_bytes(int32_t n_blocks, int32_t n_bins, int32_t max_frames,
                                         int32_t m, int32_t groups);
int ftmi_nnls_lbfgsb_start(const ftmi_nnls_lbfgsb_args *args, ftmi_stream_t stream);
int ftmi_nnls_lbfgsb_cycles(const ftmi_nnls_lbfgsb_args *args, int32_t cycles,
                            ftmi_stream_t stream);
int ftmi_nnls_lbfgsb_finish(const ftmi_nnls_lbfgsb_args *args, const int32_t *frames,
                            int32_t *status, double *info, ftmi_stream_t stream);

/* ====================================================================================
 * FastPitch transformer (models/fast_pitch.py).  Activations channels-last (B, T, C).
 * ==================================================================================== */

/* nn.Embedding + PositionalEncoding (fast_pitch.py:16-33, eval: dropout is identity):
 * out[b,t,:] = table[ids[b,t],:] + scale[0] * pe[t,:] (float32 multiply, then add).
 * pe: [T_max][dim] rows (the reference buffer (max_len, 1, dim)); scale: device float[1]. */
int ftmi_embedding_posenc(const int64_t *ids, int32_t B, int32_t T, const float *table,
                          int64_t rows, int32_t dim, const float *pe, const float *scale,
                          float *out, int32_t *err, ftmi_stream_t stream);

/* LengthRegulator (common_layers.py:12-19) fused with the postnet's PositionalEncoding:
 * y[b,t,:] = (index[b,t] >= 0 ? x[b,index[b,t],:] : 0) + scale[0] * pe[t,:].
 * x: (B, T, C) rows; index: (B, T_mel) from ftmi_lr_index; y: (B, T_mel, C) rows. */
int ftmi_lr_posenc(const float *x, int64_t x_stride, int32_t B, int32_t T, int32_t C,
                   const int32_t *index, int32_t T_mel, const float *pe, const float *scale,
                   float *y, int64_t y_stride, ftmi_stream_t stream);

/* nn.LayerNorm(C) over rows (FFTBlock.norm1/norm2 :64-65, ForwardTransformer.norm :112):
 * biased variance, y = (x*rstd - rstd*mean)*gamma + beta.  C <= 1024; y may alias x. */
int ftmi_layernorm(const float *x, int64_t x_stride, int64_t M, int32_t C, const float *gamma,
                   const float *beta, float eps, float *y, int64_t y_stride, ftmi_stream_t stream);

/* Row-panel projection (ABI 13) — the k = 1 contractions of a FastPitch FFT block
 * (models/fast_pitch.py:56-91: self_attn in_proj, out_proj + residual -> norm1, conv2 with
 * kernel 1 + residual -> norm2) with their epilogue in one launch:
 *   v = x W^T + bias (+ residual);   y = ln_gamma ? LayerNorm(v) : v
 * (nn.LayerNorm over the N columns: biased variance, eps, y = (v*rstd - rstd*mean)*gamma +
 * beta as ftmi_layernorm).  x: M rows of K floats (K % 4 == 0, 16-B aligned, x_stride % 4
 * == 0); w_split_frag: ftmi_split_weights_f16_frag of W [N][K]; N % 256 == 0, N == 256 with
 * LayerNorm; bias, residual (M x N, res_stride), ln_gamma / ln_beta (both or neither):
 * nullable.  y (M x N, y_stride) must not alias x; it may alias residual.  f16x3 arithmetic:
 * the projection values are bit-identical to ftmi_conv1d's on FTMI_MMA_F16X3 with the same
 * planes in row-major order; status bit 0 (optional word) when |x| > 65504 (rerun
 * unfused on FTMI_MMA_F32). */
int ftmi_panel_proj(const float *x, int64_t x_stride, int64_t M, int32_t K,
                    const void *w_split_frag, int32_t N, const float *bias,
                    const float *residual, int64_t res_stride, const float *ln_gamma,
                    const float *ln_beta, float eps, float *y, int64_t y_stride,
                    uint32_t *status, ftmi_stream_t stream);

/* nn.MultiheadAttention self-attention core (FFTBlock.forward :76-79; torch
 * multi_head_attention_forward math path): per batch b and head h,
 *   O = softmax((Q * qscale) K^T + mask) V,  Q/K/V = qkv[b, :, off + h*head_dim ...]
 * from the packed in_proj output rows (row stride row_stride floats; q/k/v column
 * offsets q_off/k_off/v_off).  key_padding_mask: (B, T) bytes, nonzero = padded key
 * (-inf), or NULL.  qscale = float32(sqrt(1/head_dim)).  out: (B, T, H*head_dim) rows of
 * stride out_stride.  head_dim in {64, 128}.  mma (ABI 8): FTMI_MMA_F16X3 (default: both
 * contractions on the f16x3 split, softmax fp32; an operand beyond the f16 range sets
 * FTMI_STATUS_F16_RANGE in *status, optional) or FTMI_MMA_F32 (fp32 MFMA).  workspace
 * (ABI 9, nullable): with >= ftmi_attention_workspace_bytes caller-owned bytes the f16x3
 * path splits K and V once per call into f16 planes there (instead of once per query tile
 * inside the attention kernel); results are identical. */
int64_t ftmi_attention_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t head_dim);
int ftmi_attention(const float *qkv, int64_t row_stride, int32_t B, int32_t T, int32_t H,
                   int32_t head_dim, int32_t q_off, int32_t k_off, int32_t v_off,
                   const uint8_t *key_padding_mask, float qscale, float *out,
                   int64_t out_stride, int32_t mma, uint32_t *status, void *workspace,
                   int64_t workspace_bytes, ftmi_stream_t stream);

/* ABI 14: the attention split pass folded into the in_proj projection.
 * ftmi_panel_proj_qkv = ftmi_panel_proj of self_attn.in_proj (models/fast_pitch.py:76; W
 * [3d][K], d = 256, no residual / LayerNorm) on B*T rows that writes only the Q third as fp32
 * rows (q_out, q_stride >= d) and K / V into kv_workspace (>= ftmi_attention_workspace_bytes
 * (B, T, heads, d / heads) bytes) as the f16 head / scaled-tail planes ftmi_attention's split
 * pass would write for the same values (K [B*heads][Tp][hd], V [B*heads][hd][Tp], Tp = T
 * rounded up to 64; keys T..Tp-1 are never written: the attention kernels zero them while
 * staging the last key tile, so the workspace may hold anything there — including the
 * non-finite values an earlier, overflowing call stored).
 * ftmi_attention_kv = ftmi_attention (f16x3) with Q rows q (row_stride) and K / V taken from
 * such a workspace: no split pass.  The pair computes exactly what ftmi_panel_proj +
 * ftmi_attention with a workspace compute (bit-identical); |value| > 65504 sets status bit 0. */
int ftmi_panel_proj_qkv(const float *x, int64_t x_stride, int32_t B, int32_t T, int32_t K,
                        const void *w_split_frag, int32_t d, const float *bias, int32_t heads,
                        float *q_out, int64_t q_stride, void *kv_workspace,
                        int64_t workspace_bytes, uint32_t *status, ftmi_stream_t stream);
int ftmi_attention_kv(const float *q, int64_t row_stride, int32_t B, int32_t T, int32_t H,
                      int32_t head_dim, const uint8_t *key_padding_mask, float qscale,
                      float *out, int64_t out_stride, uint32_t *status,
                      const void *kv_workspace, int64_t workspace_bytes,
                      ftmi_stream_t stream);


/* ---- WaveRNN vocoder (models/fatchord_version.py; gen_forward.py `wavernn`) -------------
 * Fixed architecture of the reference config (config.yaml:189-198): rnn_dims = fc_dims = 512,
 * feat_dims = 80, aux_dims = res_out_dims / 4 = 32; RAW with n_classes = 2^bits <= 512, or
 * MOL (n_classes = 30).  Anything else returns FTMI_E_UNSUPPORTED. */

/* One UpsampleNetwork.up_layers pair (:74-81, :88): Stretch2d(scale, 1) then
 * Conv2d(1, 1, (1, 2 scale + 1), padding (0, scale), no bias) along time, on time-major rows:
 *   y[b, j, c] = sum_i w[i] xs[j + crop0 + i - scale, c],  xs[q] = x[b, q / scale, c]
 * (zero outside [0, W scale)).  x (B, W, C) rows, y (B, W_out, C); crop0 + W_out <= W scale
 * (the final layer writes only the [indent, -indent) crop of :89). */
int ftmi_wr_stretch_conv(const float *x, int64_t x_batch_stride, int32_t B, int32_t W, int32_t C,
                         int32_t scale, const float *w, float *y, int64_t y_batch_stride,
                         int32_t W_out, int32_t crop0, ftmi_stream_t stream);

/* Arguments of ftmi_wavernn.  Weights are fp32, packed once per weights version (float64
 * products, forwardtacotron_amd/wavernn.py `_pack`):
 *   w_hh1, w_hh2 [3R][R]          rnn1/rnn2.weight_hh_l0 (gate rows r, z, n)
 *   w_ih2a [3R][R]                rnn2.weight_ih_l0[:, :R] (the x + h1 part)
 *   w_fc1a [F][R], w_fc2a [F][F]  fc1.weight[:, :R], fc2.weight[:, :F]
 *   w_fc3 [NC][F], b_fc3 [NC]     fc3
 *   b_hh1, b_hh2 [3R]             rnn1/rnn2.bias_hh_l0
 *   u1 = W_ih1 w0, u2 = W_ih2a w0 [3R], v1 = W_fc1a w0 [F]   (w0 = I.weight[:, 0]: the
 *                                 sample's column, carried through the linear layers)
 *   wm [3R + 3R + F][80]          mel columns of G1 = W_ih1 I, Q = W_ih2a I, R = W_fc1a I
 *   cond (bias_row + 1) rows of [3R | 3R | F | F] floats: per mel FRAME the aux terms of
 *                                 G1, Q (+ W_ih2b a2), R (+ W_fc1b a3), S = W_fc2b a4, with
 *                                 every bias folded in; row bias_row = biases only (padding)
 *   mel (items * item_rows, 80)   upsampled mel rows (UpsampleNetwork output)
 * Position of fold b, step t: batched: sample g = b fold_stride + t of item 0 (fold_stride
 * = target + overlap, fold_with_overlap :294-341); else g = t of item b.  g >= item_rows
 * is the fold padding (zero conditioning).  cond row = item frames_per_item + g / hop.
 * Mode: xin == NULL: generate — samples (B, L) receives each fold's drawn samples (:237 /
 * distribution.py:127 values); xin (B, L): teacher-forced forward — logits (B, L, NC).
 * seed: Philox4x32-10 key of the draws (oracle/wr_torch_cpu.py PhiloxSampler).
 * workspace: >= ftmi_wavernn_workspace_bytes() bytes, 16-B aligned (zeroed by the call). */
typedef struct {
  const float *w_hh1, *w_hh2, *w_ih2a, *w_fc1a, *w_fc2a, *w_fc3, *b_fc3, *b_hh1, *b_hh2;
  const float *u1, *u2, *v1, *wm, *cond, *mel;
  const float *xin;
  float *samples, *logits;
  void *workspace;
  uint32_t *status;
  uint64_t seed;
  int32_t bias_row, item_rows, frames_per_item, hop, fold_stride, batched;
  int32_t B, L, n_classes, mol;
  int32_t rnn_dims, fc_dims, feat_dims, aux_dims;
} ftmi_wavernn_args;

/* The sample loop of WaveRNN.generate (:203-241) — teacher-forced: WaveRNN.forward
 * (:145-169) — for B folds as persistent launches of 256 workgroups (one per CU; fewer CUs:
 * FTMI_E_UNSUPPORTED), <= 32 folds per launch.  A workgroup that cannot meet the others
 * (not co-resident) sets FTMI_STATUS_RNN_TIMEOUT in *status: the output is then invalid. */
int64_t ftmi_wavernn_workspace_bytes(void);
int ftmi_wavernn(const ftmi_wavernn_args *args, ftmi_stream_t stream);
uint32_t ftmi_set_wavernn_spin_limit(uint32_t limit);

/* One launch of the sample loop: wavernn_kernel<nbv, ni> (ni instances of up to nbv folds
 * each) over folds [fold0, fold0 + n_folds). */
typedef struct {
  int32_t nbv, ni, fold0, n_folds;
} ftmi_wr_launch;

/* Host-only (launches nothing, makes no device call): the launches ftmi_wavernn (B = n_folds)
 * and ftmi_wavernn_packed issue for n_folds folds, from the one function that decides them
 * (csrc/wavernn.hip wr_route): <= 32 folds per launch in fold order, two instances from two
 * folds on, nbv the least of 8 / 16 / 32 that holds an instance's folds.  It reads the
 * environment per call, like both entry points: FTMI_WR_NI=1 forces one instance
 * (FTMI_WR_STAMPS=1, the phase stamps, changes no launch).  *n_launches receives the count,
 * launches[0 .. min(count, capacity)) the launches (capacity 0: the count alone).
 * n_folds <= 0: FTMI_E_ARG. */
int ftmi_wavernn_route(int32_t n_folds, ftmi_wr_launch *launches, int32_t capacity,
                       int32_t *n_launches);

/* generate's tail (:246-261) in float64: samples (B, L) -> mu-law decode
 * (DSP.decode_mu_law(y, n_classes, False), utils/dsp.py:156-161; n_classes a power of two)
 * -> batched: xfade_and_unfold (:343-406), else fold 0 -> [:wave_len] -> the last fade_len
 * samples times linspace(1, 0, fade_len) (generate: fade_len = 20 hop; 0: none).
 * wave_len >= fade_len (the reference raises otherwise). */
int ftmi_wr_unfold(const float *samples, int32_t B, int32_t L, int32_t target, int32_t overlap,
                   int32_t batched, int32_t mu_law, int32_t n_classes, int32_t wave_len,
                   int32_t fade_len, double *out, ftmi_stream_t stream);

/* Packed sample loop: the folds of MANY utterances of unequal length share launches.  Each
 * fold is one row of a descriptor table in place of (fold0 + b, fold_stride, item_rows):
 *   mel_row0   first row of its utterance in `mel` (the utterances' upsampled rows, concatenated)
 *   cond_row0  first row of its utterance's frames in `cond`
 *   g0         the fold's start inside the utterance (batched: fold index * fold_stride; else 0)
 *   n_rows     the utterance's upsampled length; position g = g0 + t >= n_rows is padding
 *              (zero mel row, cond row bias_row), exactly like ftmi_wavernn's fold padding
 *   philox_b   word b of the Philox counters (t, b, k/4, .): the fold's index within ITS OWN
 *              utterance, so an utterance draws the stream it draws when run alone
 *   out_row    its row of xin / samples / logits (L floats, L * n_classes for logits)
 *   k0, k1     the utterance's Philox key (seed & 0xffffffff, seed >> 32)
 * 32 bytes a row; the table is 16-B aligned. */
typedef struct {
  int32_t mel_row0, cond_row0, g0, n_rows, philox_b, out_row;
  uint32_t k0, k1;
} ftmi_wr_fold;

/* Arguments of ftmi_wavernn_packed: the weights, cond, mel, xin / samples / logits, workspace
 * and status of ftmi_wavernn_args, and
 *   folds         n_folds descriptors.  Device memory: used as it is, its rows checked by
 *                 whoever filled it.  Host memory: every row is checked here (FTMI_E_SHAPE for
 *                 g0 < 0, g0 >= n_rows, n_rows <= 0, out_row outside [0, n_out_rows), rows
 *                 past n_mel_rows / bias_row) and the table is copied in stream order; it
 *                 must stay unchanged until the stream has passed the call.
 *   launch_steps  host array, one entry per launch (ftmi_wavernn_route's count), 1 .. L: the steps
 *                 that launch runs (rows of unequal length: its longest row); NULL: L each.
 *   L             row stride of xin / samples / logits and the default step count
 *   n_out_rows, n_mel_rows, bias_row   rows of samples, of mel, and cond's last row. */
typedef struct {
  const float *w_hh1, *w_hh2, *w_ih2a, *w_fc1a, *w_fc2a, *w_fc3, *b_fc3, *b_hh1, *b_hh2;
  const float *u1, *u2, *v1, *wm, *cond, *mel;
  const float *xin;
  float *samples, *logits;
  void *workspace;
  uint32_t *status;
  const ftmi_wr_fold *folds;
  const int32_t *launch_steps;
  int32_t n_folds, L, n_out_rows, n_mel_rows, bias_row, hop, n_classes, mol;
  int32_t rnn_dims, fc_dims, feat_dims, aux_dims;
} ftmi_wavernn_packed_args;

/* ftmi_wavernn's launches (ftmi_wavernn_route(n_folds), in table order; the same kernels and
 * hand-off protocol) over a descriptor table.  Nothing is launched when an argument or a
 * host table row is refused. */
int ftmi_wavernn_packed(const ftmi_wavernn_packed_args *args, ftmi_stream_t stream);

/* Host-only: the row check ftmi_wavernn_packed makes on a host table, for a caller that
 * hands its table over as device memory.  folds: n_folds rows in HOST memory; the other
 * arguments are the ftmi_wavernn_packed_args fields of the same names.  FTMI_OK, or
 * FTMI_E_SHAPE with the index of the first refused row in *bad_row (may be NULL);
 * folds == NULL, n_folds <= 0 or hop <= 0: FTMI_E_ARG. */
int ftmi_wr_check_folds(const ftmi_wr_fold *folds, int32_t n_folds, int32_t L, int32_t n_out_rows,
                        int32_t n_mel_rows, int32_t bias_row, int32_t hop, int32_t *bad_row);

/* One utterance of a packed sample matrix: its fold rows [first_row, first_row + n_folds),
 * its wave of wave_len float64 samples at out + out_offset. */
typedef struct {
  int32_t first_row, n_folds, wave_len, out_offset;
} ftmi_wr_item;

/* ftmi_wr_unfold for every utterance of a packed (n_rows, L) sample matrix in one launch;
 * each utterance's slice is bit-equal to ftmi_wr_unfold on its rows.  items: n_items rows,
 * 16-B aligned, device or host memory under the rule of ftmi_wavernn_packed_args.folds
 * (host rows are held to ftmi_wr_unfold's shape rules and to out_len: FTMI_E_SHAPE).
 * Unbatched: n_folds = 1.  out_len <= 2^30, n_items <= 65535 (else FTMI_E_UNSUPPORTED). */
int ftmi_wr_unfold_packed(const float *samples, int32_t n_rows, int32_t L, const ftmi_wr_item *items,
                          int32_t n_items, int32_t target, int32_t overlap, int32_t batched,
                          int32_t mu_law, int32_t n_classes, int32_t fade_len, double *out,
                          int64_t out_len, ftmi_stream_t stream);

/* Host-only: the row check ftmi_wr_unfold_packed makes on a host table (the shape rules of
 * ftmi_wr_unfold, which is the single item (0, B, wave_len, 0) with out_len = wave_len;
 * unbatched it reads fold 0 alone: n_folds = 1).  items: n_items rows in HOST memory; the
 * other arguments as in ftmi_wr_unfold_packed.  FTMI_OK, or FTMI_E_SHAPE with the index of
 * the first refused row in *bad_row (may be NULL); items == NULL or n_items <= 0: FTMI_E_ARG. */
int ftmi_wr_check_items(const ftmi_wr_item *items, int32_t n_items, int32_t n_rows, int32_t L,
                        int32_t target, int32_t overlap, int32_t batched, int32_t fade_len,
                        int64_t out_len, int32_t *bad_row);

/* ---- Tacotron decoder loop (models/tacotron.py; gen_tacotron.py, train_tacotron.py's
 * attention pass) ---------------------------------------------------------------------------
 * Fixed architecture of the reference config (config.yaml:51-61): decoder_dims = 256 (the
 * context width, 2 encoder_dims), lstm_dims = 512, n_mels = 80, decoder prenet 80 -> 256 ->
 * 128, LSA with 32 filters of 31 taps, Decoder.max_r = 20.  Anything else, more than
 * FTMI_TACO_MAX_TOKENS tokens or more than FTMI_TACO_MAX_BATCH items per call returns
 * FTMI_E_UNSUPPORTED (the host chunks larger batches). */
enum { FTMI_TACO_MAX_TOKENS = 512, FTMI_TACO_MAX_BATCH = 2, FTMI_TACO_STAMPS = 24 };

/* Arguments of ftmi_tacotron_decoder.  All weights fp32, the reference's tensors unless a
 * transposition is stated:
 *   enc, enc_proj (B, T, 256)     encoder output and encoder_proj(encoder output)
 *   pre_w1t [80][256], pre_w2t [256][128], pre_b1, pre_b2   decoder.prenet fc1 / fc2,
 *                                 weights TRANSPOSED (free-running mode only)
 *   gru_wih [768][384], gru_whh [768][256], gru_bih, gru_bhh [768]   decoder.attn_rnn
 *   lsa_conv [32][2][31], lsa_L [256][32], lsa_Lb [256], lsa_wt [256][256] = attn_net.W.weight
 *                                 TRANSPOSED, lsa_Wb [256], lsa_v [256]
 *   rin_w [512][512], rin_b [512] decoder.rnn_input
 *   l1_*, l2_*                    res_rnn1 / res_rnn2: w_ih, w_hh [2048][512], b_ih, b_hh [2048]
 *   mel_w [1600][512]             decoder.mel_proj.weight (rows mel * 20 + j, j < r, are read)
 * Mode: pre_gi == NULL: free-running generate (B = 1) — the kernel feeds the last of each
 *   step's r frames back through the prenet, applies the reference's stop rule (every value
 *   of the step's r frames < stop_threshold and t > 10, t = step * r) on the device and writes
 *   the number of decoder steps taken to *steps_out; the host reads it once after the launch.
 *   pre_gi (B, n, 768), n = ceil(steps / r): teacher-forced — row (b, s) is
 *   W_ih[:, 256:] prenet(frame s r - 1 of item b, zero for s = 0) + b_ih, computed before the
 *   launch; no stop rule, steps_out (optional) receives n.
 * steps: frames asked for (the reference's `steps` / m.size(2)); n = ceil(steps / r) decoder
 *   steps at most.  mel_out (B, n r, 80) channels-last frames, attn_out (B, n, T): rows past
 *   the steps taken are left untouched.
 * workspace: ftmi_tacotron_decoder_workspace_bytes(B, T) bytes (0: unsupported shape), 16-B
 *   aligned, zeroed by the call; one per stream. */
typedef struct ftmi_taco_args {
  const float *enc, *enc_proj;
  const float *pre_w1t, *pre_b1, *pre_w2t, *pre_b2;
  const float *gru_wih, *gru_whh, *gru_bih, *gru_bhh;
  const float *lsa_conv, *lsa_L, *lsa_Lb, *lsa_wt, *lsa_Wb, *lsa_v;
  const float *rin_w, *rin_b;
  const float *l1_wih, *l1_whh, *l1_bih, *l1_bhh;
  const float *l2_wih, *l2_whh, *l2_bih, *l2_bhh;
  const float *mel_w;
  const float *pre_gi;
  float *mel_out, *attn_out;
  int32_t *steps_out;
  uint32_t *status;
  void *workspace;
  uint64_t *stamps; /* diagnostic, normally NULL: FTMI_TACO_STAMPS device words that receive
                       workgroup 0's s_memtime sums per phase (tools/taco_stamps.py) */
  float stop_threshold;
  int32_t B, T, r, steps;
  int32_t decoder_dims, lstm_dims, n_mels, prenet_dims;
} ftmi_taco_args;

/* The decoder loop of Tacotron.generate (:304-312) / Tacotron.forward (:250-256) as ONE
 * persistent launch of 256 workgroups (one per CU, checked before the launch: fewer resident
 * returns FTMI_E_UNSUPPORTED and launches nothing).  Exact fp32 FMA arithmetic.  A workgroup
 * that cannot meet the others sets FTMI_STATUS_RNN_TIMEOUT in *status: the output is then
 * invalid.  T in [1, FTMI_TACO_MAX_TOKENS]. */
int64_t ftmi_tacotron_decoder_workspace_bytes(int32_t B, int32_t T);
int ftmi_tacotron_decoder(const ftmi_taco_args *args, ftmi_stream_t stream);

/* ---- Alignment: durations and attention scores from Tacotron's attention (the reference's
 * utils/duration_extraction.py and utils/metrics.py; train_tacotron.py:129-171) ---------------
 * att: fp32 (B, rows, T), row stride ld_row >= T, item stride ld_item (floats).  mel_len,
 * x_len: device int32 [B]; x_len NULL means T.  1 <= T <= FTMI_TACO_MAX_TOKENS (else
 * FTMI_E_UNSUPPORTED); rows is limited by the workspace only.  One workgroup per item.  The
 * kernels clamp mel_len to [1, rows] and x_len to [1, T], so no value in those arrays makes
 * them read or write out of bounds.
 *
 * ftmi_align_dijkstra (extract_durations_with_dijkstra): per item, R = mel_len[b], C = x_len[b],
 *   w[i][j] = (double)(1.0f - att[i][j]) (fp32 subtraction), D[0][0] = 0 (w[0][0] not counted),
 *   D[i][j] = w[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]) in fp64 over the predecessors
 *   that exist: the reference's grid graph (right / down / down-right edges weighted by their
 *   destination), so D equals scipy's dist_matrix bit for bit.  cost_out[b] (optional double
 *   [B]) = D[R-1][C-1].  Predecessor ties go to the first of diagonal, up, left.  Backtrack
 *   from (R-1, C-1); each row's frame is counted for the largest column the path visits in
 *   that row, so sum(dur_out[b]) == R.  dur_out: int32 (B, T), entries >= C written as 0.
 *   workspace: ftmi_align_workspace_bytes(B, rows, T) bytes (0: unsupported shape), 16-B
 *   aligned, one per stream; it need not be zeroed.
 * ftmi_align_count (extract_durations_per_count): first-index argmax of every row over the
 *   first C columns, the sequential jump repair (|a[t] - a[t-1]| > 10: a[t] = a[t-1], against
 *   the repaired predecessor), bincount of the first R entries.
 * ftmi_attention_score (attention_score): L = mel_len[b] / r, n = min(rows, L);
 *   first-index argmax over all T columns; loc_out[b] = #{1 <= t < n: |a[t] - a[t-1]| <= r}
 *   / (L - 1) (NaN for L == 1, like the reference); sharp_out[b] = (sum_{t < n} max_j
 *   att[t][j]) / rows, summed in fp64 and rounded once.  Either output may be NULL, not both. */
int64_t ftmi_align_workspace_bytes(int32_t B, int32_t rows, int32_t T);
int ftmi_align_dijkstra(const float *att, int64_t ld_row, int64_t ld_item, int32_t B, int32_t rows,
                        int32_t T, const int32_t *mel_len, const int32_t *x_len,
                        int32_t *dur_out, double *cost_out, void *workspace,
                        ftmi_stream_t stream);
int ftmi_align_count(const float *att, int64_t ld_row, int64_t ld_item, int32_t B, int32_t rows,
                     int32_t T, const int32_t *mel_len, const int32_t *x_len, int32_t *dur_out,
                     ftmi_stream_t stream);
int ftmi_attention_score(const float *att, int64_t ld_row, int64_t ld_item, int32_t B,
                         int32_t rows, int32_t T, const int32_t *mel_len, int32_t r,
                         float *loc_out, float *sharp_out, ftmi_stream_t stream);

/* ---- Phoneme-level pitch and energy from the durations (the reference's extract_pitch_energy
 * and normalize_values, train_tacotron.py:23-104) ------------------------------------------------
 * ftmi_phoneme_features: one launch over the batch, one workgroup per item, no workspace.
 *   mel: fp32 log-mel (B, n_mels, rows), unit frame stride, bin stride ld_bin >= rows, item
 *   stride ld_item (floats).  dur: int32 (B, T), row stride ld_dur >= T, 1 <= T <=
 *   FTMI_TACO_MAX_TOKENS (else FTMI_E_UNSUPPORTED).  mel_len, x_len (NULL: T): device int32 [B].
 *   pitch: fp32 (B, P) raw frame pitch, row stride ld_pitch >= P, with pitch_len int32 [B];
 *   pitch, pitch_len and pitch_out are given together or all NULL (energy only).
 *   Per item, L = mel_len[b], C = x_len[b], PL = pitch_len[b], clamped into [0, rows], [0, T],
 *   [0, P]; cum = running sum of max(dur[i], 0) over i < C; token i covers frames
 *   [min(cum[i], L), min(cum[i+1], L)).
 *     energy[t]     = sqrt(sum_k e_k * e_k), e_k = exp((double)mel[k][t]), fp64, k ascending
 *     energy_out[i] = (float)(sum of energy[t] over the token's frames, t ascending, fp64 /
 *                     their count); 0 for an empty range
 *     pitch_out[i]  = the same mean over the frames t < PL whose pitch v has v != 0.0f and
 *                     v < pitch_max_freq (both tests in fp32); 0 if none is left
 *   Tokens i >= min(C, L) get 0 in both outputs (the reference's loop visits range(mel_len)
 *   tokens only).  Frames >= L, duration columns >= C and pitch entries >= PL reach no result.
 *   dur_sum[b] = sum of dur[b][i], i < C, negative entries included, saturated to int32: the
 *   caller compares it with mel_len (the reference's assert); it is not a device status word.
 *   pitch_out, energy_out: fp32 (B, T) contiguous.  The order of every sum is fixed: an item's
 *   result does not depend on B.  Domain: finite mel values <= 40.
 * ftmi_nonzero_moments: out[0 .. 3) (device double) = the count of entries v != 0 of values[0 .. n),
 *   their mean, and their population standard deviation sqrt(sum (v - mean)^2 / count), in fp64
 *   with a fixed order of additions (1024 partials, a fixed tree): the same bits on every call.
 *   No non-zero entry: 0, 0, 0.
 * ftmi_normalize_nonzero: values[i] = (values[i] - mean) / std in place where values[i] != 0: an
 *   fp32 subtraction, then the correctly rounded fp32 quotient. */
int ftmi_phoneme_features(const float *mel, int64_t ld_bin, int64_t ld_item, int32_t B,
                          int32_t n_mels, int32_t rows, const int32_t *mel_len, const int32_t *dur,
                          int64_t ld_dur, int32_t T, const int32_t *x_len, const float *pitch,
                          int64_t ld_pitch, int32_t P, const int32_t *pitch_len,
                          float pitch_max_freq, float *pitch_out, float *energy_out,
                          int32_t *dur_sum, ftmi_stream_t stream);
int ftmi_nonzero_moments(const float *values, int64_t n, double *out, ftmi_stream_t stream);
int ftmi_normalize_nonzero(float *values, int64_t n, float mean, float std, ftmi_stream_t stream);

/* ---- Validation losses (the reference's evaluate(): trainer/common.py:69-78 MaskedL1,
 * F.l1_loss, F.cross_entropy, utils/distribution.py:16-84 discretized_mix_logistic_loss) ----------
 * Common to the three: every term and every sum is fp64, and the result is rounded to fp32 once.
 * A first launch gives each workgroup a fixed slice of the input (which slice depends on the shape
 * alone) and writes one fp64 partial per workgroup into `workspace`; a second launch of one
 * workgroup adds the partials in a fixed order (1024 strided sums, then a fixed tree) and divides.
 * No workgroup waits for another and nothing is added with atomics: the same input gives the same
 * bits on every call.  workspace: ftmi_*_workspace_bytes(...) bytes (0: unsupported shape or bad
 * sizes), 16-B aligned, one per stream; it need not be zeroed.  out: one device float.
 *
 * ftmi_l1_loss: x, target fp32 (B, C, L), each with its own item / channel / frame strides in
 *   floats.  Each operand must be frame-major (frame stride 1, channel stride >= L) or
 *   channel-major (channel stride 1, frame stride >= C), item stride >= 0; else FTMI_E_SHAPE.
 *   lens: device int32 [B] or NULL.  With lens, n_b = clamp(lens[b], 0, L) and
 *     out = sum_{b, c, t < n_b} |x - target| / (C * sum_b n_b)          (MaskedL1)
 *   sum_b n_b == 0 gives NaN, the reference's 0/0.  Elements at t >= n_b are never read, so a NaN
 *   or Inf in the padding does not reach the result; the reference multiplies by a 0/1 mask and
 *   would propagate it.  Domain: finite values where t < n_b.  Without lens,
 *     out = sum |x - target| / (B * C * L)                              (F.l1_loss)
 *   More than 2^22 workgroups (B * ceil(L / 32)) return FTMI_E_UNSUPPORTED.
 * ftmi_cross_entropy: logits fp32 (rows, C), row stride ld >= C, 1 <= C <= 65536 (more:
 *   FTMI_E_UNSUPPORTED); target int32 [rows].
 *     out = mean over rows of (m + log sum_j exp(x_j - m) - x_target), m the row maximum
 *   A label outside [0, C) adds nothing to the sum (the mean still divides by rows) and is counted
 *   in *bad_out (device int32): not a status word, the caller reads it with the loss and rejects
 *   the result if it is not 0.  Domain: finite logits.
 * ftmi_mol_loss: y_hat fp32 (rows, channels), row stride ld >= channels, channels = 3 K with
 *   1 <= K <= 32 (else FTMI_E_UNSUPPORTED): K mixture logits, K means, K log scales.  y fp32
 *   [rows].  Per row and component, with s = max(log_scale, log_scale_min), c = y - mean,
 *   i = exp(-s), h = 1 / (num_classes - 1):
 *     plus_in = i (c + h), min_in = i (c - h), mid_in = i c
 *     softplus(v) = v > 20 ? v : log1p(exp(v)), sigmoid(v) = 1 / (1 + exp(-v))
 *     log_prob = y < (float)-0.999 ? plus_in - softplus(plus_in)
 *              : y > (float)0.999  ? -softplus(min_in)
 *              : d = sigmoid(plus_in) - sigmoid(min_in), d > 1e-5 ? log(max(d, 1e-12))
 *              : mid_in - s - 2 softplus(mid_in) - log((num_classes - 1) / 2)
 *   The two tests on y are fp32 compares against the fp32 constants, as torch makes them.  The
 *   reference blends these branches with 0/1 masks; for finite operands a select gives the same
 *   value.  Then log_prob += log_softmax(logits)_k, row value v = the stabilised log-sum-exp over
 *   the K components; per_sample[row] (optional fp32 [rows]) = -v (reduce=False), out = -mean v.
 *   A row's per_sample value depends on that row alone. */
int64_t ftmi_l1_loss_workspace_bytes(int32_t B, int32_t C, int32_t L);
int ftmi_l1_loss(const float *x, int64_t xs_item, int64_t xs_chan, int64_t xs_frame,
                 const float *target, int64_t ts_item, int64_t ts_chan, int64_t ts_frame, int32_t B,
                 int32_t C, int32_t L, const int32_t *lens, float *out, void *workspace,
                 ftmi_stream_t stream);
int64_t ftmi_cross_entropy_workspace_bytes(int64_t rows, int32_t C);
int ftmi_cross_entropy(const float *logits, int64_t ld, int64_t rows, int32_t C,
                       const int32_t *target, float *out, int32_t *bad_out, void *workspace,
                       ftmi_stream_t stream);
int64_t ftmi_mol_loss_workspace_bytes(int64_t rows, int32_t K);
int ftmi_mol_loss(const float *y_hat, int64_t ld, int64_t rows, int32_t channels, const float *y,
                  double num_classes, double log_scale_min, float *out, float *per_sample,
                  void *workspace, ftmi_stream_t stream);

/* ---- Audio preparation (the reference's preprocess.py:51-91 Preprocessor._convert_file: the
 * start / end silence trim of utils/dsp.py:112-113 -> librosa 0.7.2 effects.trim, the peak rule
 * and the vocoder labels of utils/dsp.py:143-153; added under ABI 22 without a signature change) --
 * Common: y fp32 audio rows (B, L), unit sample stride, row stride y_stride >= L in floats,
 *   2 <= L < 2^31, B <= 65535 (more: FTMI_E_UNSUPPORTED).  lengths: device int32 [B] or NULL (L);
 *   an entry is clamped into [0, L] on the device, so no value can address outside the row.  No
 *   workgroup waits for another; every sum has a fixed order: the same input, the same bits.
 * ftmi_frame_power: power[b][f] for f < F (F <= 1 + L / hop; the caller passes 1 + L / hop), fp32
 *   (B, F) contiguous.  With yp = the item's L_b samples reflect-padded by frame_length / 2 on
 *   both sides (numpy.pad mode='reflect', any pad width),
 *     power[b][f] = (float)(sum_{i < frame_length} yp[f hop + i]^2 / frame_length)
 *   summed in fp64 and rounded once (librosa's rms takes a float32 mean, its square root, and
 *   squares again); frames f >= 1 + L_b / hop get 0.  frame_length even and > 0, hop >= 1, else
 *   FTMI_E_ARG.  When hop divides frame_length (at most 64 times) each sample is squared once
 *   into per-hop block sums and a frame adds frame_length / hop of them; otherwise each frame
 *   is summed directly.
 * ftmi_trim_bounds: per item, over its own frames f < 1 + L_b / hop, in fp64 from the fp32
 *   powers:  db[f] = 10 log10(max(1e-10, power[f])) - 10 log10(max(1e-10, max_f power[f])),
 *   a frame is non-silent when db[f] > -top_db;  bounds[b] = (first hop, min(L_b, (last + 1) hop))
 *   over the non-silent frames, (0, 0) if there is none.  bounds: int32 (B, 2) contiguous.
 * ftmi_peak_abs: peak[b] = max |y[b][i]| over bounds[b][0] <= i < bounds[b][1] (0 for an empty
 *   range), exact.  Zeroes peak with a memset on the stream first.  bounds are clamped into
 *   the row on the device.
 * ftmi_prepare_audio: with (s, e) = bounds[b], n = e - s:
 *     out[b][i]   = y[b][s + i] for i < n, divided by peak[b] (correctly rounded fp32 quotient)
 *                   when (peak_norm || peak[b] > 1) && peak[b] > 0 — the reference divides an
 *                   all-zero item by 0, here it stays as it is; 0 for n <= i < L
 *     new_len[b]  = n
 *     quant[b][i] (int64, optional: NULL skips the labels) for i < n, from out[b][i]:
 *       mu_law != 0: floor((fx + 1) / 2 mu + 0.5), fx = sign(x) log(1 + mu |x|) / log(1 + mu),
 *                    mu = 2^bits - 1, in fp64 from the fp32 sample (DSP.encode_mu_law)
 *       mu_law == 0: trunc(clip((x + 1) * (2^bits - 1) / 2, 0, 2^bits - 1)), three separate fp32
 *                    operations (DSP.float_2_label on float32 input); the MOL mode is bits = 16
 *       0 for n <= i < L.
 *   out (row stride out_stride >= L) must not alias y: rows move left.  bits outside 1..16:
 *   FTMI_E_UNSUPPORTED. */
int ftmi_frame_power(const float *y, int64_t y_stride, int32_t B, int64_t L, const int32_t *lengths,
                     int32_t frame_length, int32_t hop, int32_t F, float *power,
                     ftmi_stream_t stream);
int ftmi_trim_bounds(const float *power, int32_t B, int32_t F, int64_t L, const int32_t *lengths,
                     int32_t hop, double top_db, int32_t *bounds, ftmi_stream_t stream);
int ftmi_peak_abs(const float *y, int64_t y_stride, int32_t B, int64_t L, const int32_t *bounds,
                  float *peak, ftmi_stream_t stream);
int ftmi_prepare_audio(const float *y, int64_t y_stride, int32_t B, int64_t L,
                       const int32_t *bounds, const float *peak, int32_t peak_norm, int32_t mu_law,
                       int32_t bits, float *out, int64_t out_stride, int64_t *quant,
                       int64_t quant_stride, int32_t *new_len, ftmi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FTMI_H */
