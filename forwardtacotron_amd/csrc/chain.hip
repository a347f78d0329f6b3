// Launch lists (include/ftmi.h ftmi_run_chain): a chain of ftmi_* launches issued by one
// call.  Host code only: the list is validated as a whole, its references resolved against
// the base table, and the entry points called in order on the caller's stream.  Nothing is
// allocated, synchronised or kept between calls.
#include "common.h"

namespace {

// pointer roles per tag: W = the op writes through it, the minimum extent comes from its shape
struct Span {
  int slot;       // index into ftmi_chain_op::p
  int64_t bytes;  // least extent the op's shape needs behind the pointer
};

inline int64_t rows_bytes(int64_t rows, int64_t stride, int64_t width) {
  return rows > 0 ? ((rows - 1) * stride + width) * 4 : 0;
}

// the ranges `op` writes; returns their count, or -1 for an unknown tag
int written(const ftmi_chain_op &op, Span out[4]) {
  const int64_t *i = op.i;
  switch (op.tag) {
    case FTMI_CHAIN_EMBEDDING:
      out[0] = {2, i[0] * i[2] * 4};
      return 1;
    case FTMI_CHAIN_CONV1D: {
      const int64_t B = i[1], N = i[4], To = i[11] ? i[11] : i[2], sk = i[13];
      out[0] = {6, rows_bytes(B * To, i[10], N)};
      out[1] = {7, B * N * To * 4};
      out[2] = {8, sk > 1 ? sk * B * To * N * 4 : 0};
      return 3;
    }
    case FTMI_CHAIN_RNN_BIDIR:
      out[0] = {6, rows_bytes(i[1] * i[2], i[6], 2 * i[3])};
      out[1] = {8, ftmi_rnn_workspace_bytes((int32_t)i[1], (int32_t)i[3], (int32_t)i[0])};
      return 2;
    case FTMI_CHAIN_ROWDOT:
      out[0] = {3, i[1] * 4};
      return 1;
    default:
      return -1;
  }
}

int check_op(const ftmi_chain_op &op, const ftmi_chain_base *bases, int32_t n_bases) {
  Span w[4];
  const int nw = written(op, w);
  if (nw < 0) return FTMI_E_ARG;
  for (int k = 0; k < FTMI_CHAIN_PTRS; ++k) {
    const ftmi_chain_ref &r = op.p[k];
    if (r.slot < 0) continue;
    if (r.slot >= n_bases || !bases[r.slot].base) return FTMI_E_ARG;
    const int64_t size = bases[r.slot].bytes;
    if (r.offset < 0 || r.bytes < 0 || r.offset > size || r.bytes > size - r.offset)
      return FTMI_E_ARG;
    if ((r.flags & FTMI_CHAIN_ALIGN16) &&
        !ftmi_aligned16((const char *)bases[r.slot].base + r.offset))
      return FTMI_E_ALIGN;
  }
  for (int k = 0; k < nw; ++k) {
    const ftmi_chain_ref &r = op.p[w[k].slot];
    if (w[k].bytes < 0) return FTMI_E_ARG;
    if (r.slot >= 0 && r.bytes < w[k].bytes) return FTMI_E_ARG;
  }
  return FTMI_OK;
}

inline void *at(const ftmi_chain_op &op, int k, const ftmi_chain_base *bases) {
  const ftmi_chain_ref &r = op.p[k];
  return r.slot < 0 ? nullptr : (void *)((char *)bases[r.slot].base + r.offset);
}

int run_op(const ftmi_chain_op &op, const ftmi_chain_base *b, ftmi_stream_t stream) {
  const int64_t *i = op.i;
  switch (op.tag) {
    case FTMI_CHAIN_EMBEDDING:
      return ftmi_embedding((const int64_t *)at(op, 0, b), i[0], (const float *)at(op, 1, b), i[1],
                            i[2], (float *)at(op, 2, b), (int32_t *)at(op, 3, b), stream);
    case FTMI_CHAIN_CONV1D: {
      ftmi_conv_args a = {};
      a.x = (const float *)at(op, 0, b);
      a.w = (const float *)at(op, 1, b);
      a.bias = (const float *)at(op, 2, b);
      a.bn_scale = (const float *)at(op, 3, b);
      a.bn_shift = (const float *)at(op, 4, b);
      a.residual = (const float *)at(op, 5, b);
      a.y = (float *)at(op, 6, b);
      a.yt = (float *)at(op, 7, b);
      a.split_ws = (float *)at(op, 8, b);
      a.w_split = at(op, 9, b);
      a.status = (uint32_t *)at(op, 10, b);
      a.x_stride = i[0];
      a.B = (int32_t)i[1], a.T = (int32_t)i[2], a.Cin = (int32_t)i[3];
      a.N = (int32_t)i[4], a.k = (int32_t)i[5], a.pad = (int32_t)i[6];
      a.relu = (int32_t)i[7], a.maxpool = (int32_t)i[8];
      a.res_stride = i[9], a.y_stride = i[10];
      a.T_out = (int32_t)i[11], a.mma = (int32_t)i[12];
      a.split_k = (int32_t)i[13], a.x_split = (int32_t)i[14];
      return ftmi_conv1d(&a, stream);
    }
    case FTMI_CHAIN_RNN_BIDIR:
      return ftmi_rnn_bidir((int32_t)i[0], (int32_t)i[1], (int32_t)i[2], (int32_t)i[3],
                            (const float *)at(op, 0, b), i[4], (int32_t)i[5],
                            (const int32_t *)at(op, 1, b), (const float *)at(op, 2, b),
                            (const float *)at(op, 3, b), (const float *)at(op, 4, b),
                            (const int32_t *)at(op, 5, b), op.f[0], (float *)at(op, 6, b), i[6],
                            (int32_t)i[7], (uint32_t *)at(op, 7, b), at(op, 8, b), stream);
    case FTMI_CHAIN_ROWDOT:
      return ftmi_rowdot((const float *)at(op, 0, b), i[0], i[1], (int32_t)i[2],
                         (const float *)at(op, 1, b), (const float *)at(op, 2, b), op.f[0],
                         (float *)at(op, 3, b), stream);
    default:
      return FTMI_E_ARG;
  }
}

}  // namespace

extern "C" int ftmi_run_chain(const ftmi_chain_op *ops, int32_t n, const ftmi_chain_base *bases,
                              int32_t n_bases, int32_t *failed_op, ftmi_stream_t stream) {
  if (failed_op) *failed_op = -1;
  if (!ops || n <= 0 || !bases || n_bases <= 0) return FTMI_E_ARG;
  for (int32_t k = 0; k < n; ++k) {
    const int rc = check_op(ops[k], bases, n_bases);
    if (rc != FTMI_OK) {
      if (failed_op) *failed_op = k;
      return rc;
    }
  }
  for (int32_t k = 0; k < n; ++k) {
    const int rc = run_op(ops[k], bases, stream);
    if (rc != FTMI_OK) {
      if (failed_op) *failed_op = k;
      return rc;
    }
  }
  return FTMI_OK;
}
