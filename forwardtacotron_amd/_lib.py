"""ctypes binding of libftmi.so (declarations: include/ftmi.h).

The library is loaded lazily on first use.  torch is imported first so that the HIP
runtime torch ships (SONAME libamdhip64.so.7) is the one libftmi.so binds to: device
pointers and streams are then shared with torch without any interop layer.

There is no fallback: if the library is missing or fails to load, every op raises.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import torch  # noqa: F401  (must precede the dlopen, see module docstring)

from ._srchash import source_hash

_LIB_PATH = Path(os.environ.get('FTMI_LIB', Path(__file__).resolve().parent / 'libftmi.so'))
_lib = None

c_int, c_int64, c_float, c_void_p = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
P = c_void_p  # every device pointer travels as void*
# 22 still: ftmi_wavernn_packed, ftmi_wr_unfold_packed and the host-only queries
# ftmi_wavernn_route, ftmi_wr_check_folds, ftmi_wr_check_items, and the length-aware batch's
# ftmi_fill_tail, ftmi_maxpool_rows, ftmi_duration_counts_rows are new symbols; no existing
# signature or struct changed, so a caller built against the earlier 22 keeps working (the
# version is bumped on a signature change, include/ftmi.h)
ABI_VERSION = 22
MMA_F32, MMA_BF16X6, MMA_F16X3 = 0, 1, 2


class ConvArgs(ctypes.Structure):
    """Mirror of ftmi_conv_args (include/ftmi.h)."""
    _fields_ = [
        ('x', P), ('x_stride', c_int64), ('B', c_int), ('T', c_int), ('Cin', c_int),
        ('w', P), ('N', c_int), ('k', c_int), ('pad', c_int),
        ('bias', P), ('relu', c_int), ('bn_scale', P), ('bn_shift', P), ('maxpool', c_int),
        ('residual', P), ('res_stride', c_int64),
        ('y', P), ('y_stride', c_int64), ('yt', P), ('T_out', c_int), ('mma', c_int),
        ('split_k', c_int), ('split_ws', P), ('w_split', P), ('status', P), ('x_split', c_int),
    ]


class GemmRoute(ctypes.Structure):
    """Mirror of ftmi_gemm_route (include/ftmi.h): the kernel a conv / bank / highway launch
    takes, the split it requires and that split's workspace floats."""
    _fields_ = [('kernel', c_int), ('split_k', c_int), ('ws_floats', c_int64), ('pooled', c_int),
                ('band', c_int)]


# include/ftmi.h FTMI_ROUTE_*
(ROUTE_UNSUPPORTED, ROUTE_SKINNY, ROUTE_SKINNY_BANK, ROUTE_SLAB, ROUTE_SLAB_WS, ROUTE_SLAB_PF,
 ROUTE_BANK_WALK, ROUTE_BANK_HALVES, ROUTE_X6B_F16, ROUTE_X6B_BF16, ROUTE_X6, ROUTE_F32) = range(12)
ROUTE_SKINNIES = (ROUTE_SKINNY, ROUTE_SKINNY_BANK)
ROUTE_SLABS = (ROUTE_SLAB, ROUTE_SLAB_WS, ROUTE_SLAB_PF, ROUTE_BANK_WALK)


class RnnRoute(ctypes.Structure):
    """Mirror of ftmi_rnn_route_t (include/ftmi.h): kernel and grid of an ftmi_rnn_bidir call."""
    _fields_ = [(n, c_int) for n in (
        'status', 'kernel', 'cell', 'H', 'units', 'wk', 'mode', 'cst', 'nbl', 'cr', 'kseg', 'nbv',
        'threads', 'wg_per_group', 'groups', 'groups_per_pass', 'passes', 'first_blocks',
        'xcd_local', 'pad', 'psleep', 'cus')]


RNN_KERNEL_NONE, RNN_KERNEL_GEMV, RNN_KERNEL_BIDIR = range(3)  # include/ftmi.h FTMI_RNN_KERNEL_*


class WaveRNNArgs(ctypes.Structure):
    """Mirror of ftmi_wavernn_args (include/ftmi.h)."""
    _fields_ = [(n, P) for n in ('w_hh1', 'w_hh2', 'w_ih2a', 'w_fc1a', 'w_fc2a', 'w_fc3', 'b_fc3',
                                 'b_hh1', 'b_hh2', 'u1', 'u2', 'v1', 'wm', 'cond', 'mel', 'xin',
                                 'samples', 'logits', 'workspace', 'status')] + [
        ('seed', ctypes.c_uint64)] + [(n, c_int) for n in (
            'bias_row', 'item_rows', 'frames_per_item', 'hop', 'fold_stride', 'batched', 'B', 'L',
            'n_classes', 'mol', 'rnn_dims', 'fc_dims', 'feat_dims', 'aux_dims')]


class WaveRNNPackedArgs(ctypes.Structure):
    """Mirror of ftmi_wavernn_packed_args (include/ftmi.h)."""
    _fields_ = [(n, P) for n in ('w_hh1', 'w_hh2', 'w_ih2a', 'w_fc1a', 'w_fc2a', 'w_fc3', 'b_fc3',
                                 'b_hh1', 'b_hh2', 'u1', 'u2', 'v1', 'wm', 'cond', 'mel', 'xin',
                                 'samples', 'logits', 'workspace', 'status', 'folds',
                                 'launch_steps')] + [(n, c_int) for n in (
                                     'n_folds', 'L', 'n_out_rows', 'n_mel_rows', 'bias_row', 'hop',
                                     'n_classes', 'mol', 'rnn_dims', 'fc_dims', 'feat_dims', 'aux_dims')]


# columns of an ftmi_wr_fold row / an ftmi_wr_item row as int32 (k0, k1: the uint32 bit patterns)
WR_FOLD_COLS = ('mel_row0', 'cond_row0', 'g0', 'n_rows', 'philox_b', 'out_row', 'k0', 'k1')
WR_ITEM_COLS = ('first_row', 'n_folds', 'wave_len', 'out_offset')


class TacoArgs(ctypes.Structure):
    """Mirror of ftmi_taco_args (include/ftmi.h)."""
    _fields_ = [(n, P) for n in (
        'enc', 'enc_proj', 'pre_w1t', 'pre_b1', 'pre_w2t', 'pre_b2', 'gru_wih', 'gru_whh', 'gru_bih',
        'gru_bhh', 'lsa_conv', 'lsa_L', 'lsa_Lb', 'lsa_wt', 'lsa_Wb', 'lsa_v', 'rin_w', 'rin_b',
        'l1_wih', 'l1_whh', 'l1_bih', 'l1_bhh', 'l2_wih', 'l2_whh', 'l2_bih', 'l2_bhh', 'mel_w',
        'pre_gi', 'mel_out', 'attn_out', 'steps_out', 'status', 'workspace', 'stamps')] + [
        ('stop_threshold', c_float)] + [(n, c_int) for n in (
            'B', 'T', 'r', 'steps', 'decoder_dims', 'lstm_dims', 'n_mels', 'prenet_dims')]


class NnlsArgs(ctypes.Structure):
    """Mirror of ftmi_nnls_lbfgsb_args (include/ftmi.h)."""
    _fields_ = [('mel', P)] + [(n, c_int) for n in ('B', 'F', 'n_mels', 'n_bins', 'denorm')] + [
        ('blocks', P)] + [(n, c_int) for n in ('n_blocks', 'groups', 'm', 'max_frames', 'maxiter', 'dbg_stop')] + [
        (n, P) for n in ('rowvals', 'rowptr', 'rowlo', 'bin_rows', 'bin_w', 'pinv', 'workspace', 'S',
                         'active')]


CHAIN_EMBEDDING, CHAIN_CONV1D, CHAIN_RNN_BIDIR, CHAIN_ROWDOT = 1, 2, 3, 4
CHAIN_ALIGN16 = 1
CHAIN_PTRS, CHAIN_INTS, CHAIN_FLOATS = 12, 16, 2


class ChainRef(ctypes.Structure):
    """Mirror of ftmi_chain_ref (include/ftmi.h)."""
    _fields_ = [('slot', c_int), ('flags', c_int), ('offset', c_int64), ('bytes', c_int64)]


class ChainOp(ctypes.Structure):
    """Mirror of ftmi_chain_op (include/ftmi.h)."""
    _fields_ = [('tag', c_int), ('reserved', c_int), ('p', ChainRef * CHAIN_PTRS),
                ('i', c_int64 * CHAIN_INTS), ('f', c_float * CHAIN_FLOATS)]


class ChainBase(ctypes.Structure):
    """Mirror of ftmi_chain_base (include/ftmi.h)."""
    _fields_ = [('base', P), ('bytes', c_int64)]


# name -> (restype, argtypes); the exact export list of include/ftmi.h
SIGNATURES = {
    'ftmi_abi_version': (c_int, []),
    'ftmi_build_id': (ctypes.c_char_p, []),
    'ftmi_strerror': (ctypes.c_char_p, [c_int]),
    'ftmi_set_resident_cu_limit': (c_int, [c_int]),
    'ftmi_embedding': (c_int, [P, c_int64, P, c_int64, c_int64, P, P, P]),
    'ftmi_conv1d': (c_int, [ctypes.POINTER(ConvArgs), P]),
    'ftmi_conv_bank': (c_int, [P, c_int64, c_int, c_int, c_int, P, P, c_int, c_int, P, P, P, c_int64,
                               c_int, P, P]),
    'ftmi_conv_bank_split': (c_int, [P, c_int64, c_int, c_int, c_int, P, P, c_int, c_int, P, P, P,
                                     c_int64, c_int, P, c_int, P, c_int, P]),
    'ftmi_conv_bank_halves_ws_floats': (c_int64, [c_int, c_int, c_int, c_int]),
    'ftmi_conv_bank_halves_image_bytes': (c_int64, [c_int, c_int, c_int]),
    'ftmi_conv_bank_halves_image': (c_int, [P, c_int, c_int, c_int, P, P]),
    'ftmi_embed_bank': (c_int, [P, c_int, c_int, P, c_int, c_int, c_int, c_int, P, P, P, c_int64,
                                c_int, P, P]),
    'ftmi_highway': (c_int, [P, c_int64, c_int64, c_int, P, P, P, P, P, c_int64, c_int, P, P]),
    'ftmi_highway_split': (c_int, [P, c_int64, c_int64, c_int, P, P, P, P, P, c_int64, c_int, P,
                                   c_int, P, P]),
    'ftmi_conv1d_route': (c_int, [ctypes.POINTER(ConvArgs), ctypes.POINTER(GemmRoute)]),
    'ftmi_conv_bank_route': (c_int, [P, c_int64, c_int, c_int, c_int, P, P, c_int, c_int, P, P, P,
                                     c_int64, c_int, P, c_int, ctypes.POINTER(GemmRoute)]),
    'ftmi_highway_route': (c_int, [P, c_int64, c_int64, c_int, P, P, P, P, P, c_int64, c_int, P,
                                   ctypes.POINTER(GemmRoute)]),
    'ftmi_gemm_switches_digest': (ctypes.c_uint64, []),
    'ftmi_highway_stack': (c_int, [P, c_int64, c_int64, c_int, c_int, P, c_int, P, P, P, P, P,
                                   c_int, P, c_int64, P, c_int64, P, P]),
    'ftmi_highway_stack_spread_ws_bytes': (c_int64, [c_int64]),
    'ftmi_highway_stack_spread_blocks': (c_int, [c_int64]),
    'ftmi_highway_stack_spread': (c_int, [P, c_int64, c_int64, c_int, c_int, P, c_int, P, P, P, P,
                                          P, c_int, P, c_int64, P, c_int64, P, P, P]),
    'ftmi_split_weights_bytes': (c_int64, [c_int64, c_int64]),
    'ftmi_split_weights': (c_int, [P, c_int64, c_int64, P, P]),
    'ftmi_split_weights_f16_bytes': (c_int64, [c_int64, c_int64]),
    'ftmi_split_rows': (c_int, [P, c_int64, c_int64, c_int, P, c_int64, P, P]),
    'ftmi_split_weights_f16': (c_int, [P, c_int64, c_int64, P, P]),
    'ftmi_split_weights_f16_frag': (c_int, [P, c_int64, c_int64, P, P]),
    'ftmi_panel_proj': (c_int, [P, c_int64, c_int64, c_int, P, c_int, P, P, c_int64, P, P,
                                c_float, P, c_int64, P, P]),
    'ftmi_rnn_workspace_bytes': (c_int64, [c_int, c_int, c_int]),
    'ftmi_rnn_error_offset': (c_int64, [c_int]),
    'ftmi_rnn_blocks': (c_int, [c_int, c_int, c_int, c_int]),
    'ftmi_rnn_route': (c_int, [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(RnnRoute)]),
    'ftmi_rnn_switches_digest': (ctypes.c_uint64, []),
    'ftmi_set_rnn_spin_limit': (ctypes.c_uint32, [ctypes.c_uint32]),
    'ftmi_rnn_bidir': (c_int, [c_int, c_int, c_int, c_int, P, c_int64, c_int, P, P, P, P, P,
                               c_float, P, c_int64, c_int, P, P, P]),
    'ftmi_duration_counts': (c_int, [P, c_int, c_int, c_int, c_float, P, P, P, P]),
    'ftmi_duration_trunc_sum': (c_int, [P, c_int, c_int, P, P]),
    'ftmi_duration_counts_global': (c_int, [P, c_int, c_int, P, c_float, P, P, P, P]),
    'ftmi_fill_tail': (c_int, [P, c_int64, c_int, c_int, c_int, P, c_int, c_float, c_int, P]),
    'ftmi_maxpool_rows': (c_int, [P, c_int64, c_int, c_int, c_int, P, P, c_int64, P]),
    'ftmi_duration_counts_rows': (c_int, [P, c_int, c_int, P, c_int, c_float, P, P, P, P]),
    'ftmi_lr_index': (c_int, [P, c_int, c_int, c_int, P, P]),
    'ftmi_length_regulate': (c_int, [P, c_int64, c_int, c_int, c_int, P, c_int, P, c_int64, P]),
    'ftmi_series_proj_add': (c_int, [P, c_int64, c_int, c_int, c_int, P, P, P, c_float, P, P, P,
                                     c_float, P]),
    'ftmi_rowdot': (c_int, [P, c_int64, c_int64, c_int, P, P, c_float, P, P]),
    'ftmi_run_chain': (c_int, [ctypes.POINTER(ChainOp), c_int, ctypes.POINTER(ChainBase), c_int,
                               ctypes.POINTER(c_int), P]),
    'ftmi_embedding_posenc': (c_int, [P, c_int, c_int, P, c_int64, c_int, P, P, P, P, P]),
    'ftmi_lr_posenc': (c_int, [P, c_int64, c_int, c_int, c_int, P, c_int, P, P, P, c_int64, P]),
    'ftmi_layernorm': (c_int, [P, c_int64, c_int64, c_int, P, P, c_float, P, c_int64, P]),
    'ftmi_attention': (c_int, [P, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P,
                               c_float, P, c_int64, c_int, P, P, c_int64, P]),
    'ftmi_panel_proj_qkv': (c_int, [P, c_int64, c_int, c_int, c_int, P, c_int, P, c_int, P,
                                    c_int64, P, c_int64, P, P]),
    'ftmi_attention_kv': (c_int, [P, c_int64, c_int, c_int, c_int, c_int, P, c_float, P, c_int64,
                                  P, P, c_int64, P]),
    'ftmi_attention_workspace_bytes': (c_int64, [c_int, c_int, c_int, c_int]),
    'ftmi_stft': (c_int, [P, c_int64, c_int, c_int64, P, c_int, c_int, P, P, c_int, P, P, P]),
    'ftmi_mel_spectrogram': (c_int, [P, c_int64, c_int, c_int64, P, c_int, c_int, P, P, c_int, P,
                                     P, P, P, c_int, c_int, P, P]),
    'ftmi_griffinlim_stft': (c_int, [P, c_int64, c_int, c_int64, P, c_int, c_int, P, P, c_int, P,
                                     P, P, c_float, c_int, P, P]),
    'ftmi_spec_mul': (c_int, [P, P, c_int64, P, P]),
    'ftmi_unit_phases': (c_int, [P, c_int, c_int, c_int, P, P]),
    'ftmi_istft_workspace_bytes': (c_int64, [c_int, c_int, c_int]),
    'ftmi_istft': (c_int, [P, c_int, c_int, P, c_int, c_int, P, P, P, P, P, c_int64, c_int64, P]),
    'ftmi_griffinlim_iter': (c_int, [P, P, P, P, c_int, c_int, P, c_int, c_int, P, P, P, c_float,
                                     c_int, P]),
    'ftmi_istft_fused': (c_int, [P, c_int, c_int, P, c_int, c_int, P, P, P, P, c_int64, c_int64, P]),
    'ftmi_wr_stretch_conv': (c_int, [P, c_int64, c_int, c_int, c_int, c_int, P, P, c_int64, c_int,
                                     c_int, P]),
    'ftmi_wavernn_workspace_bytes': (c_int64, []),
    'ftmi_wavernn': (c_int, [ctypes.POINTER(WaveRNNArgs), P]),
    'ftmi_set_wavernn_spin_limit': (ctypes.c_uint32, [ctypes.c_uint32]),
    'ftmi_wr_unfold': (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    'ftmi_wavernn_packed': (c_int, [ctypes.POINTER(WaveRNNPackedArgs), P]),
    'ftmi_wr_unfold_packed': (c_int, [P, c_int, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_int, P, c_int64, P]),
    'ftmi_wavernn_route': (c_int, [c_int, P, c_int, ctypes.POINTER(c_int)]),
    'ftmi_wr_check_folds': (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    'ftmi_wr_check_items': (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int64,
                                    ctypes.POINTER(c_int)]),
    'ftmi_tacotron_decoder_workspace_bytes': (c_int64, [c_int, c_int]),
    'ftmi_tacotron_decoder': (c_int, [ctypes.POINTER(TacoArgs), P]),
    'ftmi_align_workspace_bytes': (c_int64, [c_int, c_int, c_int]),
    'ftmi_align_dijkstra': (c_int, [P, c_int64, c_int64, c_int, c_int, c_int, P, P, P, P, P, P]),
    'ftmi_align_count': (c_int, [P, c_int64, c_int64, c_int, c_int, c_int, P, P, P, P]),
    'ftmi_attention_score': (c_int, [P, c_int64, c_int64, c_int, c_int, c_int, P, c_int, P, P, P]),
    'ftmi_phoneme_features': (c_int, [P, c_int64, c_int64, c_int, c_int, c_int, P, P, c_int64, c_int,
                                      P, P, c_int64, c_int, P, c_float, P, P, P, P]),
    'ftmi_nonzero_moments': (c_int, [P, c_int64, P, P]),
    'ftmi_normalize_nonzero': (c_int, [P, c_int64, c_float, c_float, P]),
    'ftmi_l1_loss_workspace_bytes': (c_int64, [c_int, c_int, c_int]),
    'ftmi_l1_loss': (c_int, [P, c_int64, c_int64, c_int64, P, c_int64, c_int64, c_int64, c_int, c_int,
                             c_int, P, P, P, P]),
    'ftmi_cross_entropy_workspace_bytes': (c_int64, [c_int64, c_int]),
    'ftmi_cross_entropy': (c_int, [P, c_int64, c_int64, c_int, P, P, P, P, P]),
    'ftmi_mol_loss_workspace_bytes': (c_int64, [c_int64, c_int]),
    'ftmi_mol_loss': (c_int, [P, c_int64, c_int64, c_int, P, ctypes.c_double, ctypes.c_double, P, P,
                              P, P]),
    'ftmi_mel_nnls': (c_int, [P, c_int, c_int, P, c_int, c_int, c_int, c_int, P, P, P, P, P, P,
                              c_float, c_int, P, P]),
    'ftmi_nnls_lbfgsb_workspace_bytes': (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    'ftmi_nnls_lbfgsb_start': (c_int, [ctypes.POINTER(NnlsArgs), P]),
    'ftmi_nnls_lbfgsb_cycles': (c_int, [ctypes.POINTER(NnlsArgs), c_int, P]),
    'ftmi_nnls_lbfgsb_finish': (c_int, [ctypes.POINTER(NnlsArgs), P, P, P, P]),
    'ftmi_frame_power': (c_int, [P, c_int64, c_int, c_int64, P, c_int, c_int, c_int, P, P]),
    'ftmi_trim_bounds': (c_int, [P, c_int, c_int, c_int64, P, c_int, ctypes.c_double, P, P]),
    'ftmi_peak_abs': (c_int, [P, c_int64, c_int, c_int64, P, P, P]),
    'ftmi_prepare_audio': (c_int, [P, c_int64, c_int, c_int64, P, P, c_int, c_int, c_int, P,
                                   c_int64, P, c_int64, P, P]),
}


class FtmiError(RuntimeError):
    pass


def lib_path() -> Path:
    return _LIB_PATH


def load():
    """Load libftmi.so and bind every exported symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise FtmiError(f'libftmi.so not found at {_LIB_PATH}; run `python -m forwardtacotron_amd.build` '
                        '(there is no CPU fallback)')
    lib = ctypes.CDLL(str(_LIB_PATH), mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    if lib.ftmi_abi_version() != ABI_VERSION:
        raise FtmiError('libftmi.so ABI version mismatch')
    built, here = lib.ftmi_build_id().decode(), source_hash()
    if built != here and os.environ.get('FTMI_LIB') is None:
        raise FtmiError(f'{_LIB_PATH} was built from other sources (build id {built[:12]}, '
                        f'sources {here[:12]}): rebuild with `python -m forwardtacotron_amd.build`')
    _lib = lib
    return lib


def call(name: str, *args) -> None:
    """Invoke an ftmi entry point and raise FtmiError on a non-zero status."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.ftmi_strerror(rc).decode()
        raise FtmiError(f'{name} failed with status {rc}: {msg}')
