"""ctypes binding of libnvorbis_hip.so (include/nvorbis_hip.h).

This is the Python stand-in for the C# P/Invoke shim (no .NET in the build image): the same C ABI,
the same call sequence.  There is no fallback: if the shared library is missing it is built with
hipcc, and if that fails the import raises.
"""
import ctypes as C
import os

from . import build as _build

OK = 0
ERR_INVALID_DATA, ERR_ARGUMENT, ERR_RUNTIME, ERR_NOMEM = -1, -2, -3, -4
ERR_NOT_VORBIS, ERR_DEVICE, ERR_UNSUPPORTED, ERR_NO_GPU = -5, -6, -7, -8
PKT_EOS, PKT_RESYNC = 1, 2
PCM_F32, PCM_S16 = 0, 1  # output formats of the *_pcm synthesis calls (NVH_PCM_*)
MIX_NONE, MIX_MONO = 0, 1  # down-mixes of the *_mix synthesis calls (NVH_MIX_*)

_ERRNAMES = {
    ERR_INVALID_DATA: "InvalidDataException", ERR_ARGUMENT: "ArgumentOutOfRangeException",
    ERR_RUNTIME: "runtime fault (IndexOutOfRange/NullReference class)", ERR_NOMEM: "out of memory",
    ERR_NOT_VORBIS: "not a Vorbis stream", ERR_DEVICE: "HIP error", ERR_UNSUPPORTED: "unsupported stream",
    ERR_NO_GPU: "no HIP device (there is no CPU fallback)",
}


class NvhError(RuntimeError):
    def __init__(self, code, where=""):
        self.code = code
        extra = ""
        if code == ERR_DEVICE:
            extra = " hipError=%d" % lib().nvh_last_hip_error()
        super().__init__("%s failed: %d (%s)%s" % (where, code, _ERRNAMES.get(code, "?"), extra))


class PcmOut(C.Structure):
    """nvh_pcm_out: what a synthesis call writes -- sample format, down-mix, layout, channel map, and the destination's room."""
    _fields_ = [("format", C.c_int32), ("mix", C.c_int32), ("planar", C.c_int32), ("out_channels", C.c_int32),
                ("map", C.POINTER(C.c_int32)), ("extent", C.c_int64)]


class ResampleDesc(C.Structure):
    """nvh_resample_desc: rates, shape, destination format and the element strides of source and destination."""
    _fields_ = [("in_rate", C.c_int32), ("out_rate", C.c_int32), ("rows", C.c_int32), ("channels", C.c_int32),
                ("format", C.c_int32), ("reserved", C.c_int32), ("length", C.c_int64), ("src_length", C.c_int64),
                ("src_row_stride", C.c_int64), ("src_time_stride", C.c_int64), ("src_chan_stride", C.c_int64),
                ("dst_row_stride", C.c_int64), ("dst_time_stride", C.c_int64), ("dst_chan_stride", C.c_int64)]


RESAMPLE_TILE = 512  # NVH_RESAMPLE_TILE: consecutive outputs of one (row, channel) per workgroup step of k_resample_rows


class MelDesc(C.Structure):
    """nvh_mel_desc: the rule's parameters, the shape, and the element strides of source (row, time, channel) and destination
    (row, channel, frame, band)."""
    _fields_ = [("rate", C.c_int32), ("n_fft", C.c_int32), ("win_length", C.c_int32), ("hop", C.c_int32), ("n_mels", C.c_int32),
                ("mel_scale", C.c_int32), ("norm", C.c_int32), ("scale", C.c_int32), ("floor", C.c_float), ("rows", C.c_int32),
                ("channels", C.c_int32), ("reserved", C.c_int32), ("f_min", C.c_double), ("f_max", C.c_double),
                ("frames", C.c_int64), ("first", C.c_int64), ("src_length", C.c_int64),
                ("src_row_stride", C.c_int64), ("src_time_stride", C.c_int64), ("src_chan_stride", C.c_int64),
                ("dst_row_stride", C.c_int64), ("dst_chan_stride", C.c_int64), ("dst_frame_stride", C.c_int64),
                ("dst_band_stride", C.c_int64)]


MEL_HTK, MEL_SLANEY = 0, 1              # NVH_MEL_HTK / _SLANEY
MEL_NORM_NONE, MEL_NORM_SLANEY = 0, 1   # NVH_MEL_NORM_*
MEL_POWER, MEL_LN, MEL_DB = 0, 1, 2     # NVH_MEL_POWER / _LN / _DB
MEL_FRAMES = 4  # NVH_MEL_FRAMES: consecutive frames of one (row, channel) per workgroup of k_mel_rows


class MelFront(C.Structure):
    """nvh_mel_front: what lies between a row's samples and the transform's input -- window, triangle kind, padding, DC removal,
    pre-emphasis and gain.  MelFront() is today's front: nvh_mel_rows itself."""
    _fields_ = [("window", C.c_int32), ("triangles", C.c_int32), ("pad_mode", C.c_int32), ("remove_dc", C.c_int32),
                ("preemphasis", C.c_float), ("gain", C.c_float), ("reserved", C.c_int32 * 2)]

    def __init__(self, window=0, triangles=0, pad_mode=0, remove_dc=0, preemphasis=0.0, gain=1.0):
        super().__init__(window=window, triangles=triangles, pad_mode=pad_mode, remove_dc=remove_dc, preemphasis=preemphasis, gain=gain)


WIN_HANN, WIN_HANN_SYM, WIN_HAMMING, WIN_POVEY, WIN_RECT = 0, 1, 2, 3, 4  # NVH_WIN_*
TRI_HZ, TRI_MEL = 0, 1                                                    # NVH_TRI_*
PAD_ZERO, PAD_REFLECT = 0, 1                                              # NVH_PAD_*



class FnormDesc(C.Structure):
    """nvh_fnorm_desc: mode and axis, the shape, the rule's numbers, and the element strides of source and destination (row, channel,
    frame, band)."""
    _fields_ = [("mode", C.c_int32), ("axis", C.c_int32), ("rows", C.c_int32), ("channels", C.c_int32), ("frames", C.c_int32),
                ("bands", C.c_int32), ("eps", C.c_float), ("pad_value", C.c_float), ("range", C.c_float), ("offset", C.c_float),
                ("gain", C.c_float), ("reserved", C.c_int32),
                ("src_row_stride", C.c_int64), ("src_chan_stride", C.c_int64), ("src_frame_stride", C.c_int64),
                ("src_band_stride", C.c_int64), ("dst_row_stride", C.c_int64), ("dst_chan_stride", C.c_int64),
                ("dst_frame_stride", C.c_int64), ("dst_band_stride", C.c_int64)]


FNORM_NONE, FNORM_MEAN, FNORM_MEAN_VAR, FNORM_PEAK = 0, 1, 2, 3  # NVH_FNORM_NONE / _MEAN / _MEAN_VAR / _PEAK
FNORM_PER_BAND, FNORM_ALL = 0, 1                                 # NVH_FNORM_PER_BAND / _ALL
FNORM_RESIDENT_FLOATS = 19952  # NVH_FNORM_RESIDENT_FLOATS: (F | 1) * B up to here is normalised out of LDS


class CepDesc(C.Structure):
    """nvh_cep_desc: transform, DCT norm, delta order and window, the shape, the cepstra's count, the lifter, and the element strides
    of source (row, channel, frame, band) and destination (row, channel, frame, column)."""
    _fields_ = [("transform", C.c_int32), ("dct_norm", C.c_int32), ("order", C.c_int32), ("window", C.c_int32), ("rows", C.c_int32),
                ("channels", C.c_int32), ("frames", C.c_int32), ("bands", C.c_int32), ("ceps", C.c_int32), ("lifter", C.c_float),
                ("reserved", C.c_int32 * 2),
                ("src_row_stride", C.c_int64), ("src_chan_stride", C.c_int64), ("src_frame_stride", C.c_int64),
                ("src_band_stride", C.c_int64), ("dst_row_stride", C.c_int64), ("dst_chan_stride", C.c_int64),
                ("dst_frame_stride", C.c_int64), ("dst_col_stride", C.c_int64)]


CEP_NONE, CEP_DCT2 = 0, 1    # NVH_CEP_NONE / _DCT2
CEP_ORTHO, CEP_PLAIN = 0, 1  # NVH_CEP_ORTHO / _PLAIN
CEP_FRAMES = 24              # NVH_CEP_FRAMES: consecutive frames of one (row, channel) per work item of k_cep_rows
CEP_MAX_WINDOW = 8           # NVH_CEP_MAX_WINDOW

# symbol -> (restype, argtypes); also the list tests check against the header
_u8p, _f32p, _i64p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
_vp, _vpp, _ip = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)
SIGNATURES = {
    "nvh_version": (C.c_char_p, []),
    "nvh_last_hip_error": (C.c_int, []),
    "nvh_device_count": (C.c_int, []),
    "nvh_ctx_create": (C.c_int, [C.c_int, _vpp]),
    "nvh_ctx_destroy": (None, [_vp]),
    "nvh_ctx_set_hip_stream": (C.c_int, [_vp, _vp]),
    "nvh_ctx_synchronize": (C.c_int, [_vp]),
    "nvh_ctx_set_parse_lanes": (C.c_int, [_vp, C.c_int]),
    "nvh_dev_alloc": (C.c_int, [_vp, C.c_size_t, _vpp]),
    "nvh_dev_free": (None, [_vp, _vp]),
    "nvh_dev_upload": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "nvh_dev_download": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "nvh_measure_copy": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int, _f32p]),
    "nvh_stream_bitrates": (C.c_int, [_vp, _ip, _ip, _ip]),
    "nvh_mdct_reverse": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int64]),
    "nvh_inverse_couple": (C.c_int, [_vp, _vp, _vp, C.c_int]),
    "nvh_mode_decode": (C.c_int, [_vp, _vp, C.c_int, _vp] + [C.POINTER(C.c_int)] * 5),
    "nvh_residue_decode": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(C.c_int)]),
    "nvh_window_apply": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int64]),
    "nvh_overlap_buffers": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64]),
    "nvh_copy_buffer": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int64, _vp, C.c_int, C.POINTER(C.c_int)]),
    "nvh_stream_mode_info": (C.c_int, [_vp, C.c_int] + [C.POINTER(C.c_int)] * 3),
    "nvh_stream_codebook_info": (C.c_int, [_vp, C.c_int] + [C.POINTER(C.c_int)] * 7),
    "nvh_stream_codebook_tables": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp]),
    "nvh_stream_parse_book_info": (C.c_int, [_vp, C.c_int] + [C.POINTER(C.c_int)] * 6),
    "nvh_stream_position_state": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "nvh_stream_set_position_state": (C.c_int, [_vp, C.c_int, C.c_int64]),
    "nvh_stream_drop_pending": (C.c_int, [_vp]),
    "nvh_stream_packet_sample_count": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "nvh_stream_reset": (C.c_int, [_vp]),
    "nvh_stream_index_packets": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.POINTER(C.c_int64)]),
    "nvh_floor0_apply": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int64, _vp]),
    "nvh_floor1_apply": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int64, _vp]),
    "nvh_stream_floor_info": (C.c_int, [_vp, C.c_int] + [C.POINTER(C.c_int)] * 3),
    "nvh_mdct_tables": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp]),
    "nvh_calc_window": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp]),
    "nvh_calc_overlap": (C.c_int, [C.c_int, C.c_int, C.c_int, _ip, _ip, _ip]),
    "nvh_stream_open": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vpp]),
    "nvh_stream_close": (None, [_vp]),
    "nvh_stream_info": (C.c_int, [_vp, _ip, _ip, _ip, _ip]),
    "nvh_stream_set_clip": (C.c_int, [_vp, C.c_int]),
    "nvh_pinned_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "nvh_pinned_free": (None, [_vp]),
    "nvh_stream_set_gpu_parse": (C.c_int, [_vp, C.c_int]),
    "nvh_stream_has_clipped": (C.c_int, [_vp, _ip]),
    "nvh_stream_position": (C.c_int, [_vp, _i64p, _i64p, _ip]),
    "nvh_stream_push_packet": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, C.c_int]),
    "nvh_stream_push_packets": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "nvh_stream_push_end": (C.c_int, [_vp]),
    "nvh_stream_pending": (C.c_int, [_vp, _ip, _i64p]),
    "nvh_stream_next_segment": (C.c_int, [_vp, C.c_int]),
    "nvh_stream_segment_window": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64]),
    "nvh_stream_pending_segments": (C.c_int, [_vp, _i64p, _i64p, _i64p, C.c_int, _ip]),
    "nvh_stream_synth_segments": (C.c_int, [_vp, _i64p, _i64p, _i64p, C.c_int, _ip]),
    "nvh_stream_synth_segments_clipped": (C.c_int, [_vp, _ip, C.c_int, _ip]),
    "nvh_stream_pending_geometry": (C.c_int, [_vp, _vp, C.c_int]),
    "nvh_stream_pending_slabs": (C.c_int, [_vp, _vp, C.c_int64, _i64p, _vp, C.c_int]),
    "nvh_stream_lattice_pool": (C.c_int, [_vp, _vp, C.c_int64, _i64p]),
    "nvh_stream_vq_pool": (C.c_int, [_vp, _vp, C.c_int64, _i64p]),
    # the descriptor calls (what reader.py uses) ...
    "nvh_stream_synth_out": (C.c_int, [_vp, C.POINTER(PcmOut), _vp, _vp, _i64p]),
    "nvh_stream_synth_begin_out": (C.c_int, [_vp, C.POINTER(PcmOut), _vp, _i64p]),
    "nvh_batch_synth_out": (C.c_int, [_vp, C.POINTER(PcmOut), _vp]),
    # ... and the named calls, their shorthands
    "nvh_stream_synth_begin": (C.c_int, [_vp, _vp, C.c_int64, _i64p]),
    "nvh_stream_synth_end": (C.c_int, [_vp, _i64p]),
    "nvh_stream_synth": (C.c_int, [_vp, _vp, _vp, C.c_int64, _i64p]),
    "nvh_stream_synth_pcm": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int64, _i64p]),
    "nvh_stream_synth_begin_pcm": (C.c_int, [_vp, C.c_int, _vp, C.c_int64, _i64p]),
    "nvh_stream_synth_planar": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int64, _i64p]),
    "nvh_stream_synth_begin_planar": (C.c_int, [_vp, C.c_int, _vp, C.c_int64, _i64p]),
    "nvh_stream_synth_mix": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int64, _i64p]),
    "nvh_stream_synth_begin_mix": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int64, _i64p]),
    "nvh_channel_map_wave": (C.c_int, [C.c_int, _i32p]),
    "nvh_stream_synth_map": (C.c_int, [_vp, C.c_int, _i32p, C.c_int, _vp, _vp, C.c_int64, _i64p]),
    "nvh_stream_synth_begin_map": (C.c_int, [_vp, C.c_int, _i32p, C.c_int, _vp, C.c_int64, _i64p]),
    "nvh_stream_synth_planar_map": (C.c_int, [_vp, C.c_int, _i32p, C.c_int, _vp, _vp, C.c_int64, _i64p]),
    "nvh_stream_synth_begin_planar_map": (C.c_int, [_vp, C.c_int, _i32p, C.c_int, _vp, C.c_int64, _i64p]),
    "nvh_stream_parse_errors": (C.c_int, [_vp, _i32p, _i64p, C.c_int, _ip]),
    "nvh_batch_upload": (C.c_int, [_vp, _vpp]),
    "nvh_batch_info": (C.c_int, [_vp, _ip, _ip, _i64p, _i64p]),
    "nvh_batch_stats": (C.c_int, [_vp, _i64p]),
    "nvh_batch_kernels": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "nvh_stream_kernels": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "nvh_batch_steady_groups": (C.c_int, [_vp, _ip]),
    "nvh_stream_steady_groups": (C.c_int, [_vp, _ip]),
    "nvh_stream_pending_steady": (C.c_int, [_vp, _ip]),
    "nvh_steady_count": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _ip]),
    "nvh_batch_synth": (C.c_int, [_vp, _vp, C.c_int64]),
    "nvh_batch_synth_pcm": (C.c_int, [_vp, C.c_int, _vp, C.c_int64]),
    "nvh_batch_synth_planar": (C.c_int, [_vp, C.c_int, _vp, C.c_int64]),
    "nvh_batch_synth_mix": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int64]),
    "nvh_batch_synth_map": (C.c_int, [_vp, C.c_int, _i32p, C.c_int, _vp, C.c_int64]),
    "nvh_batch_synth_planar_map": (C.c_int, [_vp, C.c_int, _i32p, C.c_int, _vp, C.c_int64]),
    "nvh_batch_time": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _f32p, _f32p]),
    "nvh_batch_free": (None, [_vp]),
    "nvh_ogg_demux": (C.c_int, [_vp, C.c_size_t, _vp, C.c_int64, _vp, _vp, _vp, C.c_int, _ip, _i64p]),
    "nvh_ogg_demux_forward": (C.c_int, [_vp, C.c_size_t, C.c_int, _vp, C.c_int64, _vp, _vp, _vp, C.c_int, _ip, _i64p, _ip]),
    "nvh_ogg_index_open": (C.c_int, [_vp, C.c_size_t, C.c_int, C.POINTER(_vp)]),
    "nvh_ogg_index_close": (None, [_vp]),
    "nvh_ogg_index_info": (C.c_int, [_vp, _ip, _ip, _ip, _i64p, _ip]),
    "nvh_ogg_index_page": (C.c_int, [_vp, C.c_int, _i64p, _ip, _ip, _ip]),
    "nvh_ogg_seek": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _i64p, _i64p]),
    "nvh_ogg_demux_stream": (C.c_int, [_vp, C.c_size_t, C.c_int, _vp, C.c_int64, _vp, _vp, _vp, C.c_int, _ip, _i64p, _ip]),
    "nvh_ogg_index_packets": (C.c_int, [_vp, C.c_size_t, C.c_int, _vp, C.c_int64, _vp, _vp, _vp, C.c_int, _ip, _i64p, _i64p, _ip]),
    # rows at one sample rate (nvh_resample.hip)
    "nvh_resample_plan": (C.c_int, [C.c_int, C.c_int, _ip, _ip, _ip, _i64p]),
    "nvh_resample_taps": (C.c_int, [C.c_int, C.c_int, _vp, C.c_int64, _i64p]),
    "nvh_resample_rows": (C.c_int, [_vp, C.POINTER(ResampleDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nvh_resample_route": (C.c_int, [C.POINTER(ResampleDesc), _i64p]),
    # log-mel features of rows (nvh_mel.hip)
    "nvh_mel_plan": (C.c_int, [C.POINTER(MelDesc), _i64p, _i64p, _i64p]),
    "nvh_mel_tables": (C.c_int, [C.POINTER(MelDesc), _vp, _vp, _vp, C.c_int64, C.c_int64, C.c_int64, _i64p, _i64p, _i64p]),
    "nvh_mel_rows": (C.c_int, [_vp, C.POINTER(MelDesc), _vp, _vp, _vp]),
    "nvh_mel_front_check": (C.c_int, [C.POINTER(MelDesc), C.POINTER(MelFront)]),
    "nvh_mel_tables_front": (C.c_int, [C.POINTER(MelDesc), C.POINTER(MelFront), _vp, _vp, _vp, C.c_int64, C.c_int64, C.c_int64, _i64p, _i64p,
                                       _i64p]),
    "nvh_mel_rows_front": (C.c_int, [_vp, C.POINTER(MelDesc), C.POINTER(MelFront), _vp, _vp, _vp]),
    "nvh_mel_route": (C.c_int, [C.POINTER(MelDesc), C.POINTER(MelFront), _i64p]),
    # per-row normalisation of features (nvh_fnorm.hip)
    "nvh_fnorm_check": (C.c_int, [C.POINTER(FnormDesc)]),
    "nvh_fnorm_rows": (C.c_int, [_vp, C.POINTER(FnormDesc), _vp, _vp, _vp]),
    "nvh_fnorm_route": (C.c_int, [C.POINTER(FnormDesc), _i64p]),
    # cepstra and deltas of features (nvh_cep.hip)
    "nvh_cep_check": (C.c_int, [C.POINTER(CepDesc)]),
    "nvh_cep_plan": (C.c_int, [C.POINTER(CepDesc), _i64p, _i64p]),
    "nvh_cep_tables": (C.c_int, [C.POINTER(CepDesc), _vp, _vp, C.c_int64, C.c_int64, _i64p, _i64p]),
    "nvh_cep_rows": (C.c_int, [_vp, C.POINTER(CepDesc), _vp, _vp, _vp]),
    "nvh_cep_route": (C.c_int, [C.POINTER(CepDesc), _i64p]),
    # the corpus gather through RCCL's C API (nvh_comm.hip): what a host without torch.distributed binds to
    "nvh_comm_unique_id": (C.c_int, [_vp]),
    "nvh_comm_create": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "nvh_comm_destroy": (None, [_vp]),
    "nvh_comm_info": (C.c_int, [_vp, _ip, _ip]),
    "nvh_comm_allgather_i64": (C.c_int, [_vp, _i64p, C.c_int, _i64p]),
    "nvh_comm_gather_pcm": (C.c_int, [_vp, _vp, C.c_int64, _vp, _i64p, C.c_int, C.c_int]),
}

_lib = None


def lib_path():
    # NVH_LIB: load another build of the library (development aid: same-box A/B runs, tools/ab_bench.sh)
    return os.environ.get("NVH_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libnvorbis_hip.so")


def lib():
    """Load (building first if needed) the native library.  Raises if it cannot be had."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (soname libamdhip64.so.7).
        # Loading torch first makes the dynamic loader bind our NEEDED libamdhip64.so.7 to that copy;
        # the other order would map a second runtime from /opt/rocm and torch.cuda would see no device.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        path = lib_path()
        # A stale binary must never run (the .so is git-ignored but travels to the GPU box with the snapshot): the
        # library carries the hash of the sources it was built from.  The default library is rebuilt when it does not
        # match; an explicitly chosen one (NVH_LIB: debug / experiments / A-B builds) raises instead, unless
        # NVH_ALLOW_STALE=1 says the mismatch is intended (tools/ab_libs.sh compares builds of older commits).
        if os.environ.get("NVH_LIB"):
            if not os.environ.get("NVH_ALLOW_STALE") and _build.embedded_hash(path) != _build.source_hash():
                raise RuntimeError("%s was built from other sources (has %s, tree is %s): rebuild it or set NVH_ALLOW_STALE=1"
                                   % (path, _build.embedded_hash(path), _build.source_hash()))
        elif _build.needs_build(path):
            import sys
            sys.stderr.write("nvorbis_amd: %s is missing or stale (has %s, sources are %s): building\n"
                             % (path, _build.embedded_hash(path), _build.source_hash()))
            _build.build(force=True)
            if _build.needs_build(path):
                raise RuntimeError("libnvorbis_hip.so does not carry the hash of its sources after a rebuild")
        handle = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError here == ABI drift, fail loudly
            fn.restype = res
            fn.argtypes = args
        ver = handle.nvh_version().decode()
        if not os.environ.get("NVH_ALLOW_STALE") and ("nvh-src-hash=" + _build.source_hash()) not in ver:
            raise RuntimeError("loaded %s reports '%s', sources are %s" % (path, ver, _build.source_hash()))
        _lib = handle
    return _lib


def build_id():
    """'nvorbis_hip <version> (gfx950) nvh-src-hash=<hash>' of the library that is actually loaded."""
    return lib().nvh_version().decode()


def check(rc, where):
    if rc != OK:
        raise NvhError(rc, where)
    return rc
