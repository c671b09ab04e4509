"""ctypes binding of libpwv_hip.so (C ABI declared in include/pwv_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` (or ``build_library()`` here)
with ``hipcc --offload-arch=gfx950``.  There is NO fallback: if the shared object is
missing or a call fails, a ``PwvError`` is raised -- the product path never routes
through a CPU implementation.
"""
from __future__ import annotations

import ctypes
import glob
import hashlib
import os
import subprocess
from ctypes import POINTER, Structure, c_char_p, c_int, c_int64, c_size_t, c_uint64, c_void_p

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_REPO_ROOT = os.path.dirname(_PKG_DIR)
LIB_PATH = os.environ.get('PWV_LIB') or os.path.join(_PKG_DIR, 'libpwv_hip.so')   # PWV_LIB: A/B another build
CSRC = [os.path.join(_PKG_DIR, 'csrc', f) for f in ('pwv_layer.hip', 'pwv_layer_f16.hip', 'pwv_layer_h16.hip', 'pwv_misc.hip',
                                                    'pwv_stack_persist.hip', 'pwv_norm.hip', 'pwv_audio.hip', 'pwv_stream_tick.hip', 'pwv_score.hip', 'pwv_train.hip', 'pwv_train_loss.hip',
                                                    'pwv_train_varlen.hip', 'pwv_train_cond.hip', 'pwv_train_opt.hip', 'pwv_train_skip.hip',
                                                    'pwv_train_shared.hip', 'pwv_layer_stream_cond.hip', 'pwv_layer_stream_skip.hip')]

HEADER_VERSION = 301          # PWV_HIP_VERSION of include/pwv_hip.h these ctypes mirrors were written against
FIRST_FOLD_FLOATS = 2048      # PWV_FIRST_FOLD_FLOATS
VARLEN_REC_INTS = 8           # PWV_VARLEN_REC_INTS: int32 per 32-row unit of a packed batch (pwv_varlen_unit_map)
VARLEN_MIN_ROWS = 32          # the persistent launch of a packed batch needs every utterance this long
PWV_MAX_NETS = 2
PREC_F32, PREC_F16X3, PREC_F16 = 0, 1, 2
OUT_RESIDUAL, OUT_GATED = 0, 1
HEAD_IN_GATED, HEAD_IN_SKIPSUM = 0, 1

# every symbol include/pwv_hip.h declares (checked by tests/test_abi.py without a GPU)
EXPORTED_SYMBOLS = (
    'pwv_last_error', 'pwv_version', 'pwv_device_cus', 'pwv_causal_conv_f32', 'pwv_linear_f32',
    'pwv_upsample_repeat_f32', 'pwv_crop_time_f32', 'pwv_logistic_noise_f32', 'pwv_logistic_noise_stream_f32', 'pwv_logistic_noise_packed_f32',
    'pwv_iaf_front_f32',
    'pwv_layer_packed_floats', 'pwv_pack_layer_f32', 'pwv_proj_column_map', 'pwv_wavenet_layer_f32',
    'pwv_head_packed_floats', 'pwv_pack_head_f32', 'pwv_wavenet_head_f32', 'pwv_wavenet_stack_f32',
    'pwv_iaf_front_f16', 'pwv_cond_to_f16', 'pwv_tile32_floats', 'pwv_rows_to_tile32_f32', 'pwv_tile32_to_rows_f32',
    'pwv_linear_split_f32', 'pwv_cond_project_f32', 'pwv_pack_first_fold_f16x3', 'pwv_pack_first_fold_f32', 'pwv_cond_split_f16', 'pwv_range_flag', 'pwv_status_words_alloc', 'pwv_status_words_free', 'pwv_range_check_f32', 'pwv_range_stats_f32',
    'pwv_persist_workspace_bytes', 'pwv_persist_short_input', 'pwv_persist_status', 'pwv_wavenet_stack_persist_f32', 'pwv_varlen_unit_map',
    'pwv_wavenet_layer_stream_f32', 'pwv_stream_carry_f32', 'pwv_stream_tick_begin', 'pwv_stream_tick_commit',
    'pwv_stream_tick_ragged_begin', 'pwv_stream_tick_ragged_commit',
    'pwv_wav_to_mel_db_f32', 'pwv_pack_proj_f32', 'pwv_instance_norm_workspace_bytes', 'pwv_instance_norm_f32', 'pwv_channel_affine_f32', 'pwv_add_f32', 'pwv_gate_f32',
)

# the entry points of the extension headers (include/pwv_hip_mel_stream.h): in the same library, outside pwv_hip.h and its list
EXTENSION_SYMBOLS = ('pwv_wav_to_mel_db_stream_f32',)
# ... and of include/pwv_hip_live_tick.h: the streaming front-end inside a captured ragged tick
LIVE_TICK_SYMBOLS = ('pwv_live_tick_mel', 'pwv_live_tick_commit')
# ... and of include/pwv_hip_score.h: the L1 and the STFT power loss of generated audio
SCORE_SYMBOLS = ('pwv_score_workspace_bytes', 'pwv_score_f32')
# ... and of include/pwv_hip_train.h: the forward with saved activations and the backward pass
TRAIN_SYMBOLS = ('pwv_train_workspace_bytes', 'pwv_train_front_fwd_f32', 'pwv_train_layer_fwd_f32', 'pwv_train_head_fwd_f32',
                 'pwv_train_head_bwd_f32', 'pwv_train_layer_bwd_f32', 'pwv_train_front_bwd_f32')
# ... and of include/pwv_hip_train_loss.h: the loss head of training, L1 + STFT power loss and their gradient for the prediction
TRAIN_LOSS_SYMBOLS = ('pwv_train_loss_workspace_bytes', 'pwv_train_loss_f32')
# ... and of include/pwv_hip_train_varlen.h: training on packed batches of mixed-length utterances, and their loss head
TRAIN_VARLEN_SYMBOLS = ('pwv_train_varlen_front_fwd_f32', 'pwv_train_varlen_layer_fwd_f32', 'pwv_train_varlen_layer_bwd_f32',
                        'pwv_train_varlen_front_bwd_f32', 'pwv_train_loss_varlen_workspace_bytes', 'pwv_train_loss_varlen_f32')
# ... and of include/pwv_hip_train_cond.h: the layer kernels of training with a per-sample (transposed-conv) condition
TRAIN_COND_SYMBOLS = ('pwv_train_cond_workspace_bytes', 'pwv_train_cond_layer_fwd_f32', 'pwv_train_cond_layer_bwd_f32')
TRAIN_COND_MAX = 96           # PWV_TRAIN_COND_MAX: condition channels the per-sample layer kernels take
# ... and of include/pwv_hip_train_opt.h: the gradient arena (pack / unpack) and the fused Adam + EMA over it
TRAIN_OPT_SYMBOLS = ('pwv_train_opt_pack_f32', 'pwv_train_opt_unpack_f32', 'pwv_train_opt_adam_ema_f32')
# ... and of include/pwv_hip_train_skip.h: the layer and head kernels of training the skip-connection architecture
TRAIN_SKIP_SYMBOLS = ('pwv_train_skip_workspace_bytes', 'pwv_train_skip_layer_fwd_f32', 'pwv_train_skip_head_fwd_f32',
                      'pwv_train_skip_head_bwd_f32', 'pwv_train_skip_layer_bwd_f32')
# ... and of include/pwv_hip_train_shared.h: the two-output head of training the shared-net architecture, on o or on the skip sum
TRAIN_SHARED_SYMBOLS = ('pwv_train_shared_workspace_bytes', 'pwv_train_shared_head_fwd_f32', 'pwv_train_shared_head_bwd_f32')
# ... and of include/pwv_hip_stream_cond.h: the streaming layer launch with a per-sample (transposed-conv) condition
STREAM_COND_SYMBOLS = ('pwv_wavenet_layer_stream_cond_f32',)
# ... and of include/pwv_hip_stream_skip.h: the streaming layer launch with skip accumulation and the streaming causal front in front of it
STREAM_SKIP_SYMBOLS = ('pwv_wavenet_layer_stream_skip_f32', 'pwv_iaf_front_stream_f32')
TRAIN_HEAD_IN_GATED, TRAIN_HEAD_IN_SKIPSUM = 0, 1      # PWV_TRAIN_HEAD_IN_GATED, PWV_TRAIN_HEAD_IN_SKIPSUM
TRAIN_OPT_REC = 3             # PWV_TRAIN_OPT_REC: int64 per record of an arena table = {tensor address, arena offset, count}
TRAIN_OPT_CHUNK = 1024        # PWV_TRAIN_OPT_CHUNK: floats per record of a block map
TRAIN_OPT_MAX_GRID = 2048     # PWV_TRAIN_OPT_MAX_GRID: workgroups of a launch at most


class PwvError(RuntimeError):
    pass


class PwvRangeError(PwvError):
    """A split-fp16 ('f16x3') forward met an operand beyond fp16's exponent range (include/pwv_hip.h, range guard):
    its result is not trustworthy; rerun with precision='f32'."""


class PwvPersistError(PwvError):
    """A persistent stack launch gave up (csrc/pwv_stack_persist.hip: a bounded poll ran out, e.g. because another process
    held CUs and its workgroups were not all resident): its outputs are invalid.  The per-layer path is used from then on;
    rerun the forward."""


class LayerArgs(Structure):
    _fields_ = [
        ('G', c_int),
        ('x_in', c_void_p * PWV_MAX_NETS),
        ('x_out', c_void_p * PWV_MAX_NETS),
        ('packed', c_void_p * PWV_MAX_NETS),
        ('proj', c_void_p * PWV_MAX_NETS),
        ('proj_row_stride', c_int),
        ('cond', c_void_p),
        ('cond_channels', c_int),
        ('skip', c_void_p * PWV_MAX_NETS),
        ('skip_init', c_int),
        ('N', c_int), ('T', c_int), ('dilation', c_int),
        ('cond_hop', c_int), ('cond_offset', c_int), ('cond_frames', c_int),
        ('out_mode', c_int),
        ('precision', c_int),
        ('max_workgroups', c_int),
        ('x_first', c_void_p),
        ('causal_filter', c_void_p * PWV_MAX_NETS),
        ('first_fold', c_void_p * PWV_MAX_NETS),
        ('head_packed', c_void_p * PWV_MAX_NETS),
        ('head_out', c_void_p * PWV_MAX_NETS),
        ('head_q', c_int),
        ('x_limit', ctypes.c_float),
        ('range_flag', c_void_p),
    ]


class HeadArgs(Structure):
    _fields_ = [
        ('G', c_int),
        ('in_', c_void_p * PWV_MAX_NETS),
        ('packed', c_void_p * PWV_MAX_NETS),
        ('out', c_void_p * PWV_MAX_NETS),
        ('N', c_int), ('T', c_int), ('Q', c_int),
        ('in_mode', c_int),
        ('precision', c_int),
        ('max_workgroups', c_int),
    ]


class StackArgs(Structure):
    _fields_ = [
        ('G', c_int),
        ('n_layers', c_int),
        ('dilations', POINTER(c_int)),
        ('buf0', c_void_p * PWV_MAX_NETS),
        ('buf1', c_void_p * PWV_MAX_NETS),
        ('packed_layers', c_void_p * PWV_MAX_NETS),
        ('packed_layer_stride', c_size_t),
        ('proj', c_void_p * PWV_MAX_NETS),
        ('proj_row_stride', c_int),
        ('cond', c_void_p),
        ('cond_channels', c_int),
        ('skip', c_void_p * PWV_MAX_NETS),
        ('packed_head', c_void_p * PWV_MAX_NETS),
        ('out', c_void_p * PWV_MAX_NETS),
        ('Q', c_int),
        ('N', c_int), ('T', c_int),
        ('cond_hop', c_int), ('cond_offset', c_int), ('cond_frames', c_int),
        ('precision', c_int),
        ('max_workgroups', c_int),
        ('ev_begin', c_void_p * PWV_MAX_NETS),
        ('ev_end', c_void_p * PWV_MAX_NETS),
        ('x_first', c_void_p),
        ('causal_filter', c_void_p * PWV_MAX_NETS),
        ('separate_head', c_int),
        ('x_limit', ctypes.c_float),
        ('range_flag', c_void_p),
        ('first_fold', c_void_p * PWV_MAX_NETS),
    ]


class SizedStructure(Structure):
    """A struct that begins with `struct_size`: __init__ stamps it with the size of the class that is constructed."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = ctypes.sizeof(type(self))


class PersistArgs(SizedStructure):
    _fields_ = [
        ('struct_size', c_size_t),      # set by SizedStructure
        ('G', c_int),
        ('n_layers', c_int),
        ('dilations', POINTER(c_int)),
        ('x_ring', c_void_p * PWV_MAX_NETS),
        ('ring_stride', c_size_t),
        ('ring_rotation', c_int),
        ('packed_layers', c_void_p * PWV_MAX_NETS),
        ('packed_layer_stride', c_size_t),
        ('proj', c_void_p * PWV_MAX_NETS),
        ('proj_row_stride', c_int),
        ('N', c_int), ('T', c_int),
        ('cond_hop', c_int), ('cond_offset', c_int), ('cond_frames', c_int),
        ('workspace', c_void_p),
        ('workspace_bytes', c_size_t),
        ('workspace_clean', c_int),
        ('precision', c_int),
        ('max_workgroups', c_int),
        ('min_units_per_workgroup', c_int),
        ('x_first', c_void_p),
        ('causal_filter', c_void_p * PWV_MAX_NETS),
        ('x_limit', ctypes.c_float),
        ('range_flag', c_void_p),
        ('first_fold', c_void_p * PWV_MAX_NETS),
        ('status', c_void_p),
        ('tail_layer', c_void_p * PWV_MAX_NETS),
        ('tail_head', c_void_p * PWV_MAX_NETS),
        ('tail_out', c_void_p * PWV_MAX_NETS),
        ('tail_q', c_int),
        ('tail_dilation', c_int),
        ('affine_x', c_void_p),
        ('affine_out', c_void_p),
        # a packed ("varlen") batch: device int32 prefix sums, the unit records of pwv_varlen_unit_map, R on the host
        ('cu_rows', c_void_p),
        ('cu_frames', c_void_p),
        ('unit_map', c_void_p),
        ('varlen_rows', ctypes.c_longlong),
        # streaming: a pwv_stream_args (its histories and slot table), per net the HOST array of the row-history offsets of the launch's layers
        ('hist', c_void_p),
        ('hist_row_off', POINTER(c_size_t) * PWV_MAX_NETS),
    ]

class StreamArgs(SizedStructure):
    """pwv_stream_args: where a streaming layer launch finds its sessions' histories (include/pwv_hip.h, "STREAMING")."""
    _fields_ = [
        ('struct_size', c_size_t),      # set by SizedStructure
        ('hist_rd', c_void_p),
        ('hist_wr', c_void_p),
        ('block_stride', c_size_t),
        ('slot_tab', c_void_p),
        ('row_off', c_size_t * PWV_MAX_NETS),
        ('scalar_off', c_size_t),
        ('carry_tab', c_void_p),
        ('n_carry', ctypes.c_int32),
        ('cu_rows', c_void_p),          # NULL: the uniform [N, T] chunk; else device int32 [N + 1]: sessions of different chunk lengths (the ragged launch)
    ]


class StreamTickArgs(SizedStructure):
    """pwv_stream_tick_args: the device session table of a stream and the tables of one tick (include/pwv_hip.h, "A streaming TICK")."""
    _fields_ = [
        ('struct_size', c_size_t),      # set by SizedStructure
        ('sess', c_void_p),
        ('kept', c_void_p),
        ('entries', c_void_p),
        ('mel', c_void_p),
        ('n_slots', ctypes.c_int32), ('N', ctypes.c_int32), ('frames', ctypes.c_int32), ('n_mels', ctypes.c_int32),
        ('T', ctypes.c_int32),
        ('slot_tab', c_void_p),
        ('streams', c_void_p),
        ('cu_rows', c_void_p),
        ('chunk', c_void_p),
        ('words', c_void_p),
        ('counters', c_void_p),
    ]


class StreamTickRaggedArgs(SizedStructure):
    """pwv_stream_tick_ragged_args: the device session table of a stream and the tables of one RAGGED tick (include/pwv_hip.h, "A RAGGED
    streaming tick")."""
    _fields_ = [
        ('struct_size', c_size_t),      # set by SizedStructure
        ('sess', c_void_p),
        ('kept', c_void_p),
        ('entries', c_void_p),
        ('mel', c_void_p),
        ('n_slots', ctypes.c_int32), ('N', ctypes.c_int32), ('in_frames', ctypes.c_int32), ('n_mels', ctypes.c_int32),
        ('hop', ctypes.c_int32),
        ('min_frames', ctypes.c_int32),
        ('slot_tab', c_void_p),
        ('streams', c_void_p),
        ('cu_rows', c_void_p),
        ('cu_frames', c_void_p),
        ('chunk', c_void_p),
        ('words', c_void_p),
        ('counters', c_void_p),
        # optional, trailing ("STARTS"): NULL / 0 = no entry of the tick begins an utterance
        ('starts', c_void_p),           # device int64 [N, 2] = {flag, seed bits}
        ('first', c_void_p),            # device float [N, n_mels]: the first frame of a starting entry
        ('zero_block', ctypes.c_int32),  # a history block of zeros that is never written (>= 2 * n_slots)
    ]


MEL_STREAM_REC = 12           # PWV_MEL_STREAM_REC: int64 per session of a streaming mel push
# the fields of such a record, in order (include/pwv_hip_mel_stream.h)
MEL_REC_FIELDS = ('carry_first', 'carry_len', 'chunk_off', 'chunk_len', 'first_frame', 'frames', 'final_len', 'read_block', 'write_block',
                  'out_row', 'new_carry_first', 'max_word')


class MelStreamArgs(SizedStructure):
    """pwv_mel_stream_args: one ragged push of the streaming mel front-end."""
    _fields_ = [
        ('struct_size', c_size_t),      # set by SizedStructure
        ('wav', c_void_p),
        ('window', c_void_p),
        ('mel_basis', c_void_p),
        ('mel', c_void_p),
        ('state', c_void_p),
        ('max_key', c_void_p),
        ('rec', c_void_p),
        ('rec_host', c_void_p),
        ('wav_len', c_int64), ('mel_rows', c_int64),
        ('N', ctypes.c_int32), ('n_fft', ctypes.c_int32), ('hop', ctypes.c_int32), ('n_mels', ctypes.c_int32),
        ('n_blocks', ctypes.c_int32), ('n_words', ctypes.c_int32),
        ('amin', ctypes.c_float), ('max_db', ctypes.c_float), ('min_db', ctypes.c_float),
    ]


LIVE_TICK_REC = 12            # PWV_LIVE_TICK_REC: int64 per record of a live tick
# the fields of such a record, in order (include/pwv_hip_live_tick.h): the streaming record's, with the slot, the flags and the row of
# `first` where that one has the two blocks and the max word
LIVE_REC_FIELDS = ('carry_first', 'carry_len', 'chunk_off', 'chunk_len', 'first_frame', 'frames', 'final_len', 'slot', 'flags',
                   'out_row', 'new_carry_first', 'first_row')
LIVE_ACTIVE, LIVE_START, LIVE_FIRST = 1, 2, 4


class LiveTickArgs(SizedStructure):
    """pwv_live_tick_args: the front-end half of a live tick (include/pwv_hip_live_tick.h)."""
    _fields_ = [
        ('struct_size', c_size_t),      # set by SizedStructure
        ('wav', c_void_p),
        ('window', c_void_p),
        ('mel_basis', c_void_p),
        ('mel', c_void_p),
        ('first', c_void_p),
        ('state', c_void_p),
        ('max_key', c_void_p),
        ('scratch', c_void_p),
        ('sess', c_void_p),
        ('rec', c_void_p),
        ('rec_host', c_void_p),
        ('words', c_void_p),
        ('wav_cap', c_int64), ('mel_rows', c_int64),
        ('N', ctypes.c_int32), ('n_slots', ctypes.c_int32), ('n_first', ctypes.c_int32), ('n_fft', ctypes.c_int32), ('hop', ctypes.c_int32),
        ('n_mels', ctypes.c_int32),
        ('amin', ctypes.c_float), ('max_db', ctypes.c_float), ('min_db', ctypes.c_float), ('limit_db', ctypes.c_float),
    ]


SCORE_MAX_WIN = 1024          # PWV_SCORE_MAX_WIN
SCORE_TILE = 1024             # PWV_SCORE_TILE: samples per L1 partial


class ScoreArgs(SizedStructure):
    """pwv_score_args: one scoring call over n utterances, uniform or packed (include/pwv_hip_score.h)."""
    _fields_ = [
        ('struct_size', c_size_t),      # set by SizedStructure
        ('out', c_void_p),
        ('y', c_void_p),
        ('cu_rows', c_void_p),          # NULL: the uniform form
        ('n', ctypes.c_int32), ('T', ctypes.c_int32),
        ('rows', c_int64),
        ('win_length', ctypes.c_int32), ('hop_length', ctypes.c_int32),
        ('result', c_void_p),
        ('workspace', c_void_p),
        ('workspace_bytes', c_size_t),
    ]


TRAIN_RESIDUAL, TRAIN_LAST = 0, 1      # PWV_TRAIN_RESIDUAL, PWV_TRAIN_LAST


class TrainArgs(SizedStructure):
    """pwv_train_args: one training kernel call on one net (include/pwv_hip_train.h)."""
    _fields_ = ([('struct_size', c_size_t)]      # set by SizedStructure
                + [(n, ctypes.c_int32) for n in ('N', 'T', 'form', 'dilation', 'next_dilation', 'cond_hop', 'cond_offset', 'cond_frames',
                                                 'proj_row_stride', 'd_proj_row_stride', 'max_workgroups', 'accumulate')]
                + [(n, c_void_p) for n in ('in_', 'x', 'x_out', 'proj', 'y', 'causal_filter', 'filter', 'gate', 'dense', 'dense_bias',
                                           'skip', 'skip_bias', 'post1', 'post1_bias', 'post2', 'post2_bias',
                                           'd_out', 'd_mul', 'scale', 'u_next', 'v_next', 'd_o',
                                           'u', 'v', 'd_o_out', 'd_in', 'd_proj', 'd_causal_filter', 'd_filter', 'd_gate', 'd_dense', 'd_dense_bias',
                                           'd_skip', 'd_skip_bias', 'd_post1', 'd_post1_bias', 'd_post2', 'd_post2_bias', 'workspace')]
                + [('workspace_bytes', c_size_t)])


class TrainLossArgs(SizedStructure):
    """pwv_train_loss_args: the loss terms of a uniform batch and their gradient for the prediction (include/pwv_hip_train_loss.h)."""
    _fields_ = [
        ('struct_size', c_size_t),      # set by SizedStructure
        ('out', c_void_p),
        ('y', c_void_p),
        ('n', ctypes.c_int32), ('T', ctypes.c_int32),
        ('win_length', ctypes.c_int32), ('hop_length', ctypes.c_int32),
        ('weight_l1', ctypes.c_double), ('weight_power', ctypes.c_double),
        ('d_out', c_void_p),
        ('result', c_void_p),
        ('workspace', c_void_p),
        ('workspace_bytes', c_size_t),
    ]


class TrainVarlenArgs(SizedStructure):
    """pwv_train_varlen_args: one training kernel call on one net over a packed batch (include/pwv_hip_train_varlen.h): the fields of
    TrainArgs, then the packed batch."""
    _fields_ = (TrainArgs._fields_
                + [('cu_rows', c_void_p), ('cu_frames', c_void_p)]
                + [(n, ctypes.c_int32) for n in ('n', 'rows', 'proj_rows')])


class TrainCondArgs(SizedStructure):
    """pwv_train_cond_args: one layer call of training with a per-sample condition (include/pwv_hip_train_cond.h): the embedded
    pwv_train_args (its fields flat here, at the same offsets), then the condition."""
    _fields_ = (TrainArgs._fields_
                + [(n, c_void_p) for n in ('cond', 'gc_filter', 'gc_gate', 'filter_bias', 'gate_bias', 'd_cond', 'd_gc_filter', 'd_gc_gate',
                                           'd_filter_bias', 'd_gate_bias')]
                + [(n, ctypes.c_int32) for n in ('cond_channels', 'cond_row_stride', 'cond_utt_rows', 'd_cond_accumulate')])


class EmbedsTrainArgs(Structure):
    """A struct that begins with an embedded pwv_train_args, `train`, whose struct_size holds the size of the WHOLE struct; OWN: the
    names of the fields behind it.  `set` routes a name to the new fields first, then to `train`; `embed` takes a filled TrainArgs."""
    OWN = frozenset()

    def __init__(self, **kw):
        super().__init__()
        self.set(**kw)
        self.train.struct_size = ctypes.sizeof(type(self))

    def set(self, **kw):
        for k, v in kw.items():
            setattr(self if k in self.OWN else self.train, k, v)
        return self

    def embed(self, base):
        """Copy `base`, a filled TrainArgs (or the front of a struct that begins with its fields, as TrainVarlenArgs does), into
        `train`; its struct_size stays the whole struct's."""
        ctypes.memmove(ctypes.addressof(self.train), ctypes.addressof(base), ctypes.sizeof(TrainArgs))
        self.train.struct_size = ctypes.sizeof(type(self))
        return self


class TrainSkipArgs(EmbedsTrainArgs):
    """pwv_train_skip_args: one layer or head call of training the skip-connection architecture (include/pwv_hip_train_skip.h): the
    embedded pwv_train_args as `train` (the new struct has fields named like two of its own: d_skip, d_skip_bias), then the skip sum
    and the packed batch.  `set` routes a name to the new fields first, then to `train`."""
    _fields_ = ([('train', TrainArgs)]
                + [(n, c_void_p) for n in ('skip_sum', 'd_skip_sum', 'd_skip_sum_out', 'd_skip', 'd_skip_bias')]
                + [('skip_accumulate', ctypes.c_int32)]
                + [('cu_rows', c_void_p), ('cu_frames', c_void_p)]
                + [(n, ctypes.c_int32) for n in ('n', 'rows', 'proj_rows')])
    OWN = frozenset(('skip_sum', 'd_skip_sum', 'd_skip_sum_out', 'd_skip', 'd_skip_bias', 'skip_accumulate', 'cu_rows', 'cu_frames', 'n',
                     'rows', 'proj_rows'))


class TrainSharedArgs(EmbedsTrainArgs):
    """pwv_train_shared_args: one head call of training the shared-net architecture (include/pwv_hip_train_shared.h): the embedded
    pwv_train_args as `train`, then the head's input mode, the skip sum, dS and the shift plane (train.y is the scale plane).  `set`
    routes a name to the new fields first, then to `train`."""
    _fields_ = ([('train', TrainArgs), ('head_in', ctypes.c_int32)]
                + [(n, c_void_p) for n in ('skip_sum', 'd_skip_sum_out', 'y_shift')])
    OWN = frozenset(('head_in', 'skip_sum', 'd_skip_sum_out', 'y_shift'))


class TrainLossVarlenArgs(SizedStructure):
    """pwv_train_loss_varlen_args: the loss terms of a packed batch and their gradient for the prediction
    (include/pwv_hip_train_varlen.h)."""
    _fields_ = [
        ('struct_size', c_size_t),      # set by SizedStructure
        ('out', c_void_p),
        ('y', c_void_p),
        ('cu_rows', c_void_p),
        ('n', ctypes.c_int32), ('rows', ctypes.c_int32),
        ('win_length', ctypes.c_int32), ('hop_length', ctypes.c_int32),
        ('weight_l1', ctypes.c_double), ('weight_power', ctypes.c_double),
        ('d_out', c_void_p),
        ('result', c_void_p),
        ('workspace', c_void_p),
        ('workspace_bytes', c_size_t),
    ]


class TrainOptPackArgs(SizedStructure):
    """pwv_train_opt_pack_args: tensors into an arena, or an arena into the tensors (include/pwv_hip_train_opt.h)."""
    _fields_ = [
        ('struct_size', c_size_t),      # set by SizedStructure
        ('table', c_void_p),
        ('block_map', c_void_p),
        ('table_host', c_void_p),
        ('block_map_host', c_void_p),
        ('arena', c_void_p),
        ('arena_floats', c_int64),
        ('n', ctypes.c_int32), ('blocks', ctypes.c_int32),
    ]


class TrainOptAdamArgs(SizedStructure):
    """pwv_train_opt_adam_args: one Adam + EMA step over the arenas (include/pwv_hip_train_opt.h)."""
    _fields_ = [
        ('struct_size', c_size_t),      # set by SizedStructure
        ('table', c_void_p),
        ('block_map', c_void_p),
        ('table_host', c_void_p),
        ('block_map_host', c_void_p),
        ('grad', c_void_p),
        ('m', c_void_p),
        ('v', c_void_p),
        ('shadow', c_void_p),
        ('arena_floats', c_int64),
        ('n', ctypes.c_int32), ('blocks', ctypes.c_int32),
        ('lr_t', ctypes.c_double), ('beta1', ctypes.c_double), ('beta2', ctypes.c_double), ('eps', ctypes.c_double),
        ('decay', ctypes.c_double),
        ('grad_scale', ctypes.c_double),
    ]


# per-source extra flags (none in the product; tools/probes/regw/README.md: the register-stationary probe kernel needs
# `-mllvm -amdgpu-mfma-vgpr-form=1`, which is why the sources are compiled one by one)
EXTRA_FLAGS = {}
# extra sources for probe builds: PWV_EXTRA_SRC="path[:flag,flag...] ..."
for _e in os.environ.get('PWV_EXTRA_SRC', '').split():
    _src, _, _fl = _e.partition(':')
    CSRC.append(os.path.abspath(_src))
    EXTRA_FLAGS[os.path.basename(_src)] = [f for f in _fl.split(',') if f]


OBJ_DIR = os.path.join(_PKG_DIR, 'csrc', '_obj')


def _digest(parts) -> str:
    return hashlib.sha256('\0'.join(parts).encode()).hexdigest()[:16]


def _hipcc() -> str:
    return os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def device_compile_command(src: str) -> list:
    """The shipped compile command of one source, without its mode (-c, -S, ...), input and output: build_library derives its own
    from it, and the tests that look at resource remarks or assembly compile what ships."""
    # ONE gfx950 code object for the XNACK mode an MI355X runs in by default (xnack-): code built for a known mode instead of
    # 'either' is 0.5 % faster on the bench step; xnack+ objects (XNACK-on runs) are not available on the GPU pool
    return ([_hipcc(), '--offload-arch=gfx950:xnack-', '-O3', '-std=c++17', '-I' + os.path.join(_REPO_ROOT, 'include'), '-I' + os.path.join(_PKG_DIR, 'csrc')]
            + EXTRA_FLAGS.get(os.path.basename(src), []) + os.environ.get('PWV_CXXFLAGS', '').split())


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 into the in-tree shared library: one object per source, compiled in parallel.

    An object is named after a hash of its whole compile command (HIPCC, flags, EXTRA_FLAGS, PWV_CXXFLAGS) and reused while it is
    newer than its source and the headers; the library is rebuilt unless the hash of its link command, kept next to the objects,
    matches.  Objects and the library are written under temporary names and renamed into place, and builders in different
    processes take turns on a lock file, so no process links or loads a half-written file."""
    import fcntl
    from concurrent.futures import ThreadPoolExecutor
    if os.environ.get('PWV_LIB'):
        return LIB_PATH            # an explicitly chosen library is never rebuilt
    # every header and body of csrc/, by pattern: a new part can never be missing from the staleness check
    hdrs = glob.glob(os.path.join(_PKG_DIR, 'csrc', '*.h')) + glob.glob(os.path.join(_PKG_DIR, 'csrc', '*.inc')) + glob.glob(os.path.join(_REPO_ROOT, 'include', '*.h'))
    hdr_time = max(os.path.getmtime(h) for h in hdrs + [os.path.abspath(__file__)])
    compiles = []                  # (source, object, command without the output)
    for src in CSRC:
        cmd = device_compile_command(src) + ['-fPIC', '-c', src]
        compiles.append((src, os.path.join(OBJ_DIR, '%s.%s.o' % (os.path.basename(src), _digest(cmd))), cmd))
    link = [_hipcc(), '--offload-arch=gfx950:xnack-', '-shared', '-fPIC'] + [o for _, o, _ in compiles]
    link_hash = _digest(link)
    stamp = os.path.join(OBJ_DIR, os.path.basename(LIB_PATH) + '.inputs')
    newest = max([hdr_time] + [os.path.getmtime(s) for s in CSRC])

    def fresh():
        try:
            with open(stamp) as f:
                return f.read().strip() == link_hash and os.path.getmtime(LIB_PATH) >= newest
        except OSError:
            return False

    if not force and fresh():
        return LIB_PATH
    os.makedirs(OBJ_DIR, exist_ok=True)
    with open(os.path.join(OBJ_DIR, '.lock'), 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)          # one builder at a time; the others then find its result fresh
        if not force and fresh():
            return LIB_PATH

        def run(cmd, out):
            tmp = '%s.tmp%d' % (out, os.getpid())
            if verbose:
                print(' '.join(cmd + ['-o', out]))
            res = subprocess.run(cmd + ['-o', tmp], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if res.returncode != 0:
                if os.path.exists(tmp):
                    os.remove(tmp)
                return res.stdout
            os.replace(tmp, out)
            return None

        def compile_one(job):
            src, obj, cmd = job
            if not force and os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(src), hdr_time):
                return None
            return run(cmd, obj)

        # the GPU hosts show the whole machine's CPUs; a build gets 16 of them at most
        jobs = min(len(compiles), 16, int(os.environ.get('MAX_JOBS') or 16), os.cpu_count() or 4)
        with ThreadPoolExecutor(max_workers=max(jobs, 1)) as ex:
            errors = [e for e in ex.map(compile_one, compiles) if e is not None]
        if errors:
            raise PwvError('hipcc failed:\n' + errors[0])
        err = run(link, LIB_PATH)
        if err is not None:
            raise PwvError('hipcc (link) failed:\n' + err)
        with open(stamp + '.tmp', 'w') as f:
            f.write(link_hash + '\n')
        os.replace(stamp + '.tmp', stamp)
    return LIB_PATH


_lib = None


def _declare(lib):
    f32p = c_void_p
    lib.pwv_last_error.restype = c_char_p
    lib.pwv_last_error.argtypes = []
    lib.pwv_version.restype = c_int
    lib.pwv_device_cus.restype = c_int
    lib.pwv_causal_conv_f32.argtypes = [f32p, f32p, f32p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]
    lib.pwv_linear_f32.argtypes = [f32p, f32p, f32p, f32p, c_int, c_int, c_int, c_int, c_void_p]
    lib.pwv_linear_split_f32.argtypes = lib.pwv_linear_f32.argtypes
    lib.pwv_upsample_repeat_f32.argtypes = [f32p, f32p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]
    lib.pwv_crop_time_f32.argtypes = [f32p, f32p, c_int, c_int, c_int, c_int, c_int, c_void_p]
    lib.pwv_logistic_noise_f32.argtypes = [f32p, c_int64, c_uint64, c_uint64, c_void_p]
    lib.pwv_iaf_front_f32.argtypes = [f32p, f32p, f32p, c_int, f32p, c_int, POINTER(c_void_p), POINTER(c_void_p),
                                      c_int, c_int, c_int, c_int, c_void_p]
    lib.pwv_iaf_front_f16.argtypes = lib.pwv_iaf_front_f32.argtypes
    lib.pwv_cond_to_f16.argtypes = [f32p, c_void_p, c_int, c_int, c_int, c_void_p]
    lib.pwv_cond_split_f16.argtypes = lib.pwv_cond_to_f16.argtypes
    lib.pwv_tile32_floats.restype = c_size_t
    lib.pwv_tile32_floats.argtypes = [c_int64, c_int]
    lib.pwv_rows_to_tile32_f32.argtypes = [f32p, f32p, c_int64, c_int, c_void_p]
    lib.pwv_tile32_to_rows_f32.argtypes = [f32p, f32p, c_int64, c_int, c_void_p]
    lib.pwv_layer_packed_floats.restype = c_size_t
    lib.pwv_layer_packed_floats.argtypes = [c_int, c_int]
    lib.pwv_pack_layer_f32.argtypes = [f32p] * 8 + [c_int, c_int, c_int, f32p, c_void_p]
    lib.pwv_proj_column_map.argtypes = [POINTER(c_int)]
    lib.pwv_wavenet_layer_f32.argtypes = [POINTER(LayerArgs), c_void_p]
    lib.pwv_wavenet_layer_stream_f32.argtypes = [POINTER(LayerArgs), POINTER(StreamArgs), c_void_p]
    lib.pwv_wavenet_layer_stream_cond_f32.argtypes = [POINTER(LayerArgs), POINTER(StreamArgs), c_void_p]
    lib.pwv_wavenet_layer_stream_skip_f32.argtypes = [POINTER(LayerArgs), POINTER(StreamArgs), c_void_p]
    lib.pwv_iaf_front_stream_f32.argtypes = [f32p, c_int, POINTER(c_void_p), POINTER(c_void_p), c_int, c_int, POINTER(StreamArgs), c_void_p]
    lib.pwv_stream_carry_f32.argtypes = [POINTER(StreamArgs), c_int, c_int, c_void_p]
    lib.pwv_stream_tick_begin.argtypes = [POINTER(StreamTickArgs), c_void_p]
    lib.pwv_stream_tick_commit.argtypes = [POINTER(StreamTickArgs), c_void_p]
    lib.pwv_stream_tick_ragged_begin.argtypes = [POINTER(StreamTickRaggedArgs), c_void_p]
    lib.pwv_stream_tick_ragged_commit.argtypes = [POINTER(StreamTickRaggedArgs), c_void_p]
    lib.pwv_head_packed_floats.restype = c_size_t
    lib.pwv_head_packed_floats.argtypes = [c_int]
    lib.pwv_pack_head_f32.argtypes = [f32p] * 6 + [c_int, c_int, f32p, c_void_p]
    lib.pwv_pack_first_fold_f16x3.argtypes = [f32p, f32p, f32p, f32p, c_void_p]
    lib.pwv_pack_first_fold_f32.argtypes = [f32p, f32p, f32p, f32p, c_void_p]
    lib.pwv_wavenet_head_f32.argtypes = [POINTER(HeadArgs), c_void_p]
    lib.pwv_wavenet_stack_f32.argtypes = [POINTER(StackArgs), POINTER(c_void_p)]
    lib.pwv_pack_proj_f32.argtypes = [f32p, f32p, f32p, f32p, c_int, c_int, c_int, f32p, f32p, c_void_p]
    lib.pwv_wav_to_mel_db_f32.argtypes = [f32p, f32p, f32p, f32p, c_int, c_int, c_int, c_int, c_int] + [ctypes.c_float] * 4 + [c_int, c_void_p]
    lib.pwv_wav_to_mel_db_stream_f32.argtypes = [POINTER(MelStreamArgs), c_void_p]
    lib.pwv_live_tick_mel.argtypes = [POINTER(LiveTickArgs), c_void_p]
    lib.pwv_live_tick_commit.argtypes = [POINTER(LiveTickArgs), c_void_p]
    lib.pwv_score_workspace_bytes.restype = c_size_t
    lib.pwv_score_workspace_bytes.argtypes = [POINTER(ScoreArgs)]
    lib.pwv_score_f32.argtypes = [POINTER(ScoreArgs), c_void_p]
    lib.pwv_train_workspace_bytes.restype = c_size_t
    lib.pwv_train_workspace_bytes.argtypes = [POINTER(TrainArgs)]
    for name in TRAIN_SYMBOLS[1:]:
        getattr(lib, name).argtypes = [POINTER(TrainArgs), c_void_p]
    lib.pwv_train_loss_workspace_bytes.restype = c_size_t
    lib.pwv_train_loss_workspace_bytes.argtypes = [POINTER(TrainLossArgs)]
    lib.pwv_train_loss_f32.argtypes = [POINTER(TrainLossArgs), c_void_p]
    for name in TRAIN_VARLEN_SYMBOLS[:4]:
        getattr(lib, name).argtypes = [POINTER(TrainVarlenArgs), c_void_p]
    lib.pwv_train_loss_varlen_workspace_bytes.restype = c_size_t
    lib.pwv_train_loss_varlen_workspace_bytes.argtypes = [POINTER(TrainLossVarlenArgs)]
    lib.pwv_train_loss_varlen_f32.argtypes = [POINTER(TrainLossVarlenArgs), c_void_p]
    lib.pwv_train_cond_workspace_bytes.restype = c_size_t
    lib.pwv_train_cond_workspace_bytes.argtypes = [POINTER(TrainCondArgs)]
    for name in TRAIN_COND_SYMBOLS[1:]:
        getattr(lib, name).argtypes = [POINTER(TrainCondArgs), c_void_p]
    lib.pwv_train_skip_workspace_bytes.restype = c_size_t
    lib.pwv_train_skip_workspace_bytes.argtypes = [POINTER(TrainSkipArgs)]
    for name in TRAIN_SKIP_SYMBOLS[1:]:
        getattr(lib, name).argtypes = [POINTER(TrainSkipArgs), c_void_p]
    lib.pwv_train_shared_workspace_bytes.restype = c_size_t
    lib.pwv_train_shared_workspace_bytes.argtypes = [POINTER(TrainSharedArgs)]
    for name in TRAIN_SHARED_SYMBOLS[1:]:
        getattr(lib, name).argtypes = [POINTER(TrainSharedArgs), c_void_p]
    lib.pwv_train_opt_pack_f32.argtypes = [POINTER(TrainOptPackArgs), c_void_p]
    lib.pwv_train_opt_unpack_f32.argtypes = [POINTER(TrainOptPackArgs), c_void_p]
    lib.pwv_train_opt_adam_ema_f32.argtypes = [POINTER(TrainOptAdamArgs), c_void_p]
    lib.pwv_instance_norm_workspace_bytes.restype = c_size_t
    lib.pwv_instance_norm_workspace_bytes.argtypes = [c_int, c_int, c_int]
    lib.pwv_instance_norm_f32.argtypes = [f32p, f32p, c_int, c_int, c_int, f32p, f32p, ctypes.c_float, c_void_p, c_size_t, c_void_p]
    lib.pwv_channel_affine_f32.argtypes = [f32p, f32p, c_int64, c_int, f32p, f32p, c_int, c_int, c_void_p]
    lib.pwv_add_f32.argtypes = [f32p, f32p, f32p, c_int64, c_void_p]
    lib.pwv_gate_f32.argtypes = [f32p, f32p, f32p, c_int64, c_void_p]
    lib.pwv_persist_workspace_bytes.restype = c_size_t
    lib.pwv_persist_workspace_bytes.argtypes = [POINTER(PersistArgs)]
    lib.pwv_persist_short_input.restype = c_int
    lib.pwv_persist_short_input.argtypes = [POINTER(PersistArgs)]
    lib.pwv_persist_status.argtypes = [POINTER(c_void_p)]
    lib.pwv_wavenet_stack_persist_f32.argtypes = [POINTER(PersistArgs), c_void_p]
    lib.pwv_varlen_unit_map.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]
    lib.pwv_range_stats_f32.argtypes = [f32p] * 8 + [c_int, f32p, c_void_p]
    lib.pwv_range_flag.argtypes = [POINTER(c_void_p)]
    lib.pwv_logistic_noise_stream_f32.argtypes = [f32p, c_int64, c_void_p, c_void_p]
    lib.pwv_logistic_noise_packed_f32.argtypes = [f32p, c_void_p, c_void_p, c_int, c_int64, c_void_p]
    lib.pwv_cond_project_f32.argtypes = [f32p, f32p, c_int, f32p, f32p, f32p, f32p, c_int, c_int, c_int, ctypes.c_float, c_void_p, c_void_p]
    lib.pwv_status_words_alloc.argtypes = [POINTER(c_void_p)]
    lib.pwv_status_words_free.argtypes = [c_void_p]
    lib.pwv_range_check_f32.argtypes = [f32p, c_int64, ctypes.c_float, c_void_p, c_void_p]
    for name in EXPORTED_SYMBOLS + EXTENSION_SYMBOLS + LIVE_TICK_SYMBOLS + SCORE_SYMBOLS + TRAIN_SYMBOLS + TRAIN_LOSS_SYMBOLS + TRAIN_VARLEN_SYMBOLS + TRAIN_COND_SYMBOLS + TRAIN_OPT_SYMBOLS + TRAIN_SKIP_SYMBOLS + TRAIN_SHARED_SYMBOLS + STREAM_COND_SYMBOLS + STREAM_SKIP_SYMBOLS:      # fails loudly (AttributeError) if a symbol is missing
        getattr(lib, name)
    return lib


def lib():
    """Load libpwv_hip.so (once).  Raises PwvError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PwvError('libpwv_hip.so not built at %s -- run `python -c "import __graft_entry__ as g; '
                           'g.build()"` (hipcc, gfx950). There is no CPU fallback.' % LIB_PATH)
        # One HIP runtime per process: torch bundles its own libamdhip64.so.7 (same SONAME as
        # /opt/rocm's).  Load torch's first so our NEEDED entry binds to the runtime that owns the
        # device context, streams and allocations we are handed.
        import torch
        hip_rt = os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so')
        if os.path.exists(hip_rt):
            ctypes.CDLL(hip_rt, mode=ctypes.RTLD_GLOBAL)
        try:
            loaded = _declare(ctypes.CDLL(LIB_PATH))
        except OSError as e:
            raise PwvError('cannot load %s: %s' % (LIB_PATH, e))
        # a major version step changes an argument struct's layout (include/pwv_hip.h): never call across one
        if loaded.pwv_version() // 100 != HEADER_VERSION // 100:
            raise PwvError('%s is version %d, this binding was written against %d: rebuild it (`python -c "import __graft_entry__ as g; g.build()"`)'
                           % (LIB_PATH, loaded.pwv_version(), HEADER_VERSION))
        _lib = loaded
    return _lib


def check(code: int, what: str = ''):
    if code != 0:
        msg = lib().pwv_last_error()
        raise PwvError('%s failed (%d): %s' % (what or 'libpwv_hip call', code, msg.decode() if msg else '?'))


def proj_column_map():
    arr = (c_int * 128)()
    check(lib().pwv_proj_column_map(arr), 'pwv_proj_column_map')
    return list(arr)
