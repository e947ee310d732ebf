"""ctypes binding of include/hevcbitstream_amd.h over torch device tensors."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

# layout of hbs_nal_entry / hbs_summary (include/hevcbitstream_amd.h)
NAL_ENTRY = np.dtype([("start", "<u8"), ("end", "<u8"), ("rbsp_off", "<u8"),
                      ("rbsp_len", "<u4"), ("status", "<i4")])
SUMMARY = np.dtype([("nal_count", "<u8"), ("nal_found", "<u8"), ("rbsp_bytes", "<u8"),
                    ("stream_bytes", "<u8"), ("stop_reason", "<i4"), ("error", "<i4"),
                    ("reserved", "<u8", (3,))])
ST_ERROR, ST_TRAILING03, ST_UNTERMINATED = 1, 2, 4
# layout of hbs_nal_filter and the masks of its keep_types (hbs_filter_annexb)
NAL_FILTER = np.dtype([("keep_types", "<u8"), ("max_temporal_id_plus1", "<i4"), ("max_layer_id", "<i4"),
                       ("keep_short", "<i4"), ("reserved", "<i4")])
NALMASK_VCL = 0x00000000FFFFFFFF            # types 0..31
NALMASK_IRAP = 0x0000000000FF0000           # types 16..23
NALMASK_PARAM_SETS = 0x0000000700000000     # types 32..34
NALMASK_SEI = 0x0000018000000000            # types 39, 40
NALMASK_ALL = 0xFFFFFFFFFFFFFFFF
# layout of hbs_access_unit / hbs_au_carry and the flags of hbs_access_units / hbs_au_keep
ACCESS_UNIT = np.dtype([("first_nal", "<u8"), ("unit_begin", "<u8"), ("unit_end", "<u8"), ("nal_count", "<u4"), ("vcl_count", "<u4"),
                        ("first_vcl", "<u4"), ("nal_unit_type", "<i4"), ("temporal_id_plus1", "<i4"), ("pic_order_cnt", "<i4"),
                        ("poc_lsb", "<i4"), ("slice_types", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
AU_CARRY = np.dtype([("flags", "<u4"), ("anchor_poc_lsb", "<i4"), ("anchor_poc_msb", "<i4"), ("reserved", "<u4")])
AU_IRAP, AU_IDR, AU_CVS_START, AU_ANCHOR, AU_NO_PICTURE, AU_DAMAGED, AU_PARAM_SETS, AU_END_OF_SEQ = 1, 2, 4, 8, 16, 32, 64, 128
AUKEEP_PARAM_SETS = 1
# layout of hbs_au_times_params, the flags and the span limit of hbs_au_times
AU_TIMES_PARAMS = np.dtype([("flags", "<u4"), ("tick", "<u4"), ("base_time", "<u8"), ("delay", "<u4"), ("reserved", "<u4", (3,))])
AUT_MAX_SPAN = 1024
AUT_DELAY_GIVEN, AUT_WRAP33 = 1, 2
# layouts of hbs_cenc_subsample, hbs_cenc_plan_params and hbs_cenc_params; the flag and the scheme of the two hbs_cenc_* calls
CENC_SUBSAMPLE = np.dtype([("clear", "<u4"), ("protect", "<u4")])
CENC_PLAN_PARAMS = np.dtype([("length_size", "<i4"), ("flags", "<u4"), ("clear_lead", "<u4"), ("reserved", "<u4")])
CENC_PARAMS = np.dtype([("key", "u1", (16,)), ("iv0", "u1", (16,)), ("scheme", "<u4"), ("iv_mode", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
CENC_ALIGN16 = 1
CENC_SCHEME_CENC = 0x63656E63
# layout of hbs_cbcs_params and the flags of hbs_cbcs_crypt
CBCS_PARAMS = np.dtype([("key", "u1", (16,)), ("iv0", "u1", (16,)), ("iv_mode", "<u4"), ("flags", "<u4"), ("crypt_byte_block", "u1"),
                        ("skip_byte_block", "u1"), ("reserved0", "<u2"), ("reserved1", "<u4")])
CBCS_DECRYPT = 1
CBCS_WHOLE_RUNS = 2
# flags of hbs_au_insert
AUINS_AUD, AUINS_PARAM_SETS, AUINS_PARAM_SETS_FIRST = 1, 2, 4
# layout of hbs_ts_pes / hbs_ts_packet, the packet classes and the flags of hbs_ts_demux
TS_PES = np.dtype([("out_off", "<u8"), ("pts", "<u8"), ("dts", "<u8"), ("packet", "<u4"), ("flags", "<u4")])
TS_PACKET = np.dtype([("cls", "<i4"), ("pid", "<u4"), ("off", "<u4"), ("len", "<u4"), ("es_off", "<u4"), ("es_len", "<u4"),
                      ("cc", "<u4"), ("flags", "<u4"), ("pts", "<u8"), ("dts", "<u8")])
TS_FAULT, TS_OTHER, TS_SKIPPED, TS_NO_PAYLOAD, TS_PAYLOAD, TS_PES_START = -1, 0, 1, 2, 3, 4
TS_F_PTS, TS_F_DTS, TS_F_RANDOM_ACCESS, TS_F_DISCONTINUITY, TS_F_DATA_ALIGNED = 1, 2, 4, 8, 16
TS_NO_TIME = (1 << 64) - 1
STREAM_TYPE_HEVC = 0x24
# layout of hbs_ts_mux_params and the flags of hbs_ts_mux
TS_MUX_PARAMS = np.dtype([("packet_bytes", "<i4"), ("pid", "<i4"), ("pmt_pid", "<i4"), ("program_number", "<i4"),
                          ("transport_stream_id", "<i4"), ("flags", "<u4"), ("cc_es", "<u4"), ("cc_pat", "<u4"), ("cc_pmt", "<u4"),
                          ("reserved", "<u4"), ("pcr_lead", "<u8")])
TSMUX_PCR, TSMUX_PSI_AT_IRAP, TSMUX_NO_PSI = 1, 2, 4
# layout of hbs_rtp_params / hbs_rtp_packet, the flags of hbs_rtp_pack and the packet kinds of hbs_rtp_packet_host
RTP_PARAMS = np.dtype([("max_payload", "<i4"), ("payload_type", "<i4"), ("framing", "<i4"), ("flags", "<u4"), ("ssrc", "<u4"),
                       ("seq", "<u4"), ("ts_base", "<u4"), ("ts_step", "<u4")])
RTP_PACKET = np.dtype([("payload_off", "<u8"), ("payload_len", "<u8"), ("nal_off", "<u8"), ("nal_len", "<u8"), ("kind", "<i4"),
                       ("nal_type", "<i4"), ("marker", "<u4"), ("payload_type", "<u4"), ("seq", "<u4"), ("timestamp", "<u4"),
                       ("ssrc", "<u4"), ("fu_start", "<u4"), ("fu_end", "<u4"), ("nal_header", "u1", (2,)), ("reserved", "u1", (2,))])
RTP_OPEN_END = 1
RTP_AGGREGATE = 4         # consecutive small NALs of an access unit share an aggregation packet ...
RTP_AP_SPAN = 256         # ... which never reaches across a multiple of this in the call's NAL numbering
RTP_SINGLE, RTP_FU, RTP_AP, RTP_OTHER = 0, 1, 2, 3
# layout of hbs_rtp_unpack_params and the flags of hbs_rtp_unpack
RTP_UNPACK_PARAMS = np.dtype([("payload_type", "<i4"), ("startcode_bytes", "<i4"), ("flags", "<u4"), ("ssrc", "<u4")])
RTPU_MATCH_SSRC = 1
# layout of hbs_rtp_order_params and the flags of hbs_rtp_order
RTP_ORDER_PARAMS = np.dtype([("payload_type", "<i4"), ("flags", "<u4"), ("ssrc", "<u4"), ("reserved", "<u4"), ("max_span", "<u8"),
                             ("after_ext", "<u8")])
RTPO_MATCH_SSRC, RTPO_AFTER = 1, 2
# layout of hbs_mp4_params / hbs_mp4_frag / hbs_mp4_init_params, the flags of hbs_mp4_fragment and hbs_mp4_init_host
MP4_PARAMS = np.dtype([("length_size", "<i4"), ("flags", "<u4"), ("track_id", "<u4"), ("sequence", "<u4"), ("max_samples", "<u4"),
                       ("sample_duration", "<u4"), ("base_time", "<u8")])
MP4_FRAG = np.dtype([("out_off", "<u8"), ("out_bytes", "<u8"), ("first_au", "<u8"), ("decode_time", "<u8"), ("samples", "<u4"),
                     ("sequence", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
MP4_INIT_PARAMS = np.dtype([("track_id", "<u4"), ("timescale", "<u4"), ("width", "<u4"), ("height", "<u4"), ("length_size", "<i4"),
                            ("chroma_format_idc", "<i4"), ("bit_depth_luma", "<i4"), ("bit_depth_chroma", "<i4")])
MP4_CUT_AT_IRAP = 1
MP4_HEV1 = 1
MP4_PROTECT_PARAMS = np.dtype([("iv_size", "<u4"), ("flags", "<u4"), ("reserved", "<u4", (6,))])
MP4_TENC = np.dtype([("scheme", "<u4"), ("crypt_byte_block", "u1"), ("skip_byte_block", "u1"), ("iv_size", "u1"), ("constant_iv_size", "u1"),
                     ("kid", "u1", (16,)), ("constant_iv", "u1", (16,)), ("reserved", "<u4", (6,))])
MP4_SENC_PARAMS = np.dtype([("iv_size", "<u4"), ("track_id", "<u4"), ("flags", "<u4"), ("reserved", "<u4", (5,))])
MP4_SENC_CLEAR_IF_ABSENT = 1
MP4_SCHEME_CENC = 0x63656E63      # 'cenc'
MP4_SCHEME_CBCS = 0x63626373      # 'cbcs'
# layout of hbs_mp4_read_params / hbs_mp4_track (hbs_mp4_samples, hbs_mp4_init_read_host)
MP4_READ_PARAMS = np.dtype([("flags", "<u4"), ("track_id", "<u4"), ("trex_duration", "<u4"), ("trex_size", "<u4"), ("trex_flags", "<u4"),
                            ("reserved", "<u4", (3,))])
MP4_TRACK = np.dtype([("track_id", "<u4"), ("timescale", "<u4"), ("width", "<u4"), ("height", "<u4"), ("length_size", "<i4"),
                      ("entry", "<u4"), ("trex_duration", "<u4"), ("trex_size", "<u4"), ("trex_flags", "<u4"), ("n_nals", "<u4"),
                      ("hvcc_off", "<u8"), ("hvcc_bytes", "<u8"), ("reserved", "<u4", (2,))])
# layout of hbs_parsed_nal
WRITTEN = np.dtype([("rc", "<i4"), ("rbsp_size", "<u4"), ("slice_data_size", "<i4"), ("pad", "<u4")])
PARSED = np.dtype([("rc", "<i4"), ("nal_unit_type", "<i4"), ("nal_layer_id", "<i4"), ("nal_temporal_id_plus1", "<i4"),
                   ("struct_off", "<u8"), ("slice_data_size", "<i4"), ("slice_data_off", "<u4")])

# layout of hbs_slice_compact: sixteen members of hevc_slice_header_t, by name
COMPACT_FIELDS = ("first_slice_segment_in_pic_flag", "no_output_of_prior_pics_flag", "pic_parameter_set_id", "dependent_slice_segment_flag",
                  "slice_segment_address", "slice_type", "pic_output_flag", "slice_pic_order_cnt_lsb",
                  "short_term_ref_pic_set_sps_flag", "short_term_ref_pic_set_idx", "num_long_term_pics", "slice_temporal_mvp_enabled_flag",
                  "num_ref_idx_l0_active_minus1", "num_ref_idx_l1_active_minus1", "slice_qp_delta", "num_entry_point_offsets")
COMPACT = np.dtype([(f, "<i4") for f in COMPACT_FIELDS])

SEI_MAX_MESSAGES = 6
EXT_NAL = np.dtype([("num_sei_messages", "<i4"), ("primary_pic_type", "<i4"), ("filler_bytes", "<u4"), ("reserved", "<u4"),
                    ("sei", [("payloadType", "<i4"), ("payloadSize", "<i4"), ("payload_off", "<u4"), ("reserved", "<u4")], (SEI_MAX_MESSAGES,))])

# layout of hbs_mp4_stbl (hbs_mp4_stbl_find_host, hbs_mp4_stbl_samples): each box reference is (off, bytes)
MP4_STBL = np.dtype([("stsz", "<u8", (2,)), ("stco", "<u8", (2,)), ("stsc", "<u8", (2,)), ("stts", "<u8", (2,)), ("ctts", "<u8", (2,)),
                     ("stss", "<u8", (2,)), ("flags", "<u4"), ("reserved0", "<u4"), ("file_bytes", "<u8"), ("reserved", "<u8", (2,))])
MP4_STBL_CO64 = 1
# layout of hbs_mp4_stbl_write_params (hbs_mp4_stbl_write)
MP4_STBL_WRITE_PARAMS = np.dtype([("flags", "<u4"), ("max_chunk_samples", "<u4"), ("sample_duration", "<u4"), ("reserved0", "<u4"),
                                  ("base_time", "<u8"), ("data_offset", "<u8")])

EXPORTS = ["hbs_version", "hbs_ctx_create", "hbs_ctx_destroy", "hbs_ctx_set_stream", "hbs_ctx_use_own_stream",
           "hbs_ctx_get_stream",
           "hbs_ctx_synchronize", "hbs_last_error", "hbs_index_extract", "hbs_index_extract_host", "hbs_read_summary",
           "hbs_workspace_bytes", "hbs_write_headers", "hbs_parse_headers_trace", "hbs_emit_annexb", "hbs_annexb_bound", "hbs_synth_rbsp",
           "hbs_synth_rbsp_bound", "hbs_ctx_enable_timing", "hbs_ctx_kernel_ms", "hbs_ctx_kernel_ms_back", "hbs_ctx_grid",
           "hbs_parse_headers", "hbs_ctx_set_kernel", "hbs_ctx_set_count_ahead", "hbs_ctx_get_kernel", "hbs_ctx_last_kernel",
           "hbs_host_alloc", "hbs_host_free", "hbs_copy_to_device_async", "hbs_copy_device",
           "hbs_ctx_set_sequential_parse", "hbs_ctx_set_emit_path", "hbs_parse_extended",
           "hbs_comm_unique_id", "hbs_comm_create", "hbs_comm_adopt", "hbs_comm_destroy", "hbs_comm_rank", "hbs_comm_world", "hbs_comm_reserve_hint", "hbs_parse_headers_compact", "hbs_parse_materialize", "hbs_index_parse_compact", "hbs_gather_parts", "hbs_index_parse", "hbs_ctx_reserve_workgroups",
           "hbs_gather_index", "hbs_ctx_device", "hbs_find_cut_host", "hbs_trim_part", "hbs_annexb_bound_gaps", "hbs_ctx_device_bytes", "hbs_ctx_set_ingest_window_max", "hbs_pair_alloc", "hbs_pair_free", "hbs_pair_pool_trim", "hbs_pair_pool_stats", "hbs_parse_headers_state", "hbs_ctx_last_emit_by_tiles", "hbs_ctx_set_device_exclusive",
           "hbs_filter_annexb", "hbs_access_units", "hbs_au_keep", "hbs_au_sps_poc_offset", "hbs_au_times",
           "hbs_cenc_subsamples", "hbs_cenc_crypt", "hbs_cbcs_crypt",
           "hbs_annexb_to_lenpref", "hbs_lenpref_to_annexb",
           "hbs_ts_demux", "hbs_ts_packet_host", "hbs_ts_find_pid_host",
           "hbs_ts_mux", "hbs_ts_mux_psi_host", "hbs_ts_mux_au_packets_host",
           "hbs_au_insert", "hbs_aud_nal_host",
           "hbs_rtp_pack", "hbs_rtp_nal_packets_host", "hbs_rtp_packet_host", "hbs_rtp_ap_units_host",
           "hbs_rtp_unpack", "hbs_rtp_frames_host", "hbs_rtp_order",
           "hbs_mp4_fragment", "hbs_mp4_fragment_bytes_host", "hbs_mp4_init_host",
           "hbs_mp4_samples", "hbs_mp4_init_read_host", "hbs_mp4_stbl_samples", "hbs_mp4_stbl_find_host",
           "hbs_mp4_track_read_host",
           "hbs_mp4_stbl_write", "hbs_mp4_stbl_write_bytes_host", "hbs_mp4_moov_host",
           "hbs_mp4_protect", "hbs_mp4_protect_bytes_host", "hbs_mp4_init_protect_host",
           "hbs_mp4_senc_samples", "hbs_mp4_init_unprotect_host"]


PAIR_REPORT = np.dtype([("chunks", "<u4"), ("probed", "<u4"), ("rejected", "<u4"), ("accepted_fast", "<u4"),
                        ("unprobed_after_budget", "<u4"), ("from_pool", "<u4"), ("from_table", "<u4"), ("reserved", "<u4")])


class _PairedMemory:
    """memory from hbs_pair_alloc, handed to torch through __cuda_array_interface__; given back when the last tensor on it dies"""

    def __init__(self, lib, ptr, nbytes):
        self.lib, self.ptr = lib, ptr
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}

    def __del__(self):
        try:
            if self.ptr:
                self.lib.hbs_pair_free(None, C.c_void_p(self.ptr))
                self.ptr = 0
        except Exception:
            pass


class HbsError(RuntimeError):
    pass


def library_path():
    # HBS_LIB: a development build of the same library (make variant NAME=...), for A/B timing only
    return os.environ.get("HBS_LIB") or os.path.join(_HERE, "libhevcbitstream_amd.so")


def source_digest():
    """sha256 over the kernel sources (csrc/*.hip, *.h, *.c, sorted by name): profiles record it, and bench.py quotes a
    profile's counter figures only while it still matches (a changed kernel must be profiled again)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(_HERE, "csrc", "*"))):
        if f.endswith((".hip", ".h", ".c")):
            h.update(os.path.basename(f).encode())
            h.update(open(f, "rb").read())
    return h.hexdigest()


_lib = None


class _DevLibrary:
    """HBS_LIB only (A/B timing against a development build, possibly an older round's): an entry point the build lacks
    becomes a stub that raises when CALLED, instead of failing the load.  Never used for the shipped library."""

    def __init__(self, lib):
        self.__dict__["_lib"] = lib

    def __getattr__(self, name):
        try:
            return getattr(self._lib, name)
        except AttributeError:
            class _Missing:
                argtypes = None
                restype = None

                def __call__(self, *a):
                    raise HbsError("%s: not in the development build %s" % (name, os.environ["HBS_LIB"]))
            m = _Missing()
            self.__dict__[name] = m
            return m


def load_library():
    """Load the gfx950 library.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    p = library_path()
    if not os.path.exists(p):
        raise HbsError("%s not built: run `make lib` (hipcc --offload-arch=gfx950); "
                       "there is no CPU fallback" % p)
    lib = C.CDLL(p)
    if os.environ.get("HBS_LIB"):
        lib = _DevLibrary(lib)
    lib.hbs_version.restype = C.c_char_p
    lib.hbs_ctx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    lib.hbs_ctx_destroy.argtypes = [C.c_void_p]
    lib.hbs_ctx_destroy.restype = None
    lib.hbs_ctx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.hbs_ctx_use_own_stream.argtypes = [C.c_void_p]
    lib.hbs_ctx_get_stream.argtypes = [C.c_void_p]
    lib.hbs_ctx_get_stream.restype = C.c_void_p
    lib.hbs_ctx_synchronize.argtypes = [C.c_void_p]
    lib.hbs_ctx_enable_timing.argtypes = [C.c_void_p, C.c_int]
    lib.hbs_ctx_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    lib.hbs_ctx_kernel_ms_back.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    lib.hbs_ctx_grid.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.hbs_ctx_set_kernel.argtypes = [C.c_void_p, C.c_int]
    lib.hbs_ctx_get_kernel.argtypes = [C.c_void_p]
    lib.hbs_ctx_last_kernel.argtypes = [C.c_void_p]
    lib.hbs_last_error.argtypes = [C.c_void_p]
    lib.hbs_last_error.restype = C.c_char_p
    lib.hbs_index_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                      C.c_void_p, C.c_uint64, C.c_void_p]
    lib.hbs_index_extract_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                           C.c_void_p, C.c_uint64, C.c_void_p]
    lib.hbs_write_headers.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_uint32, C.c_void_p]
    lib.hbs_read_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hbs_workspace_bytes.argtypes = [C.c_uint64]
    lib.hbs_workspace_bytes.restype = C.c_uint64
    lib.hbs_emit_annexb.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int,
                                    C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.hbs_annexb_bound.argtypes = [C.c_uint64, C.c_uint64]
    lib.hbs_annexb_bound.restype = C.c_uint64
    lib.hbs_synth_rbsp.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64,
                                   C.c_void_p, C.c_void_p]
    lib.hbs_parse_headers.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                      C.c_uint64, C.c_void_p]
    lib.hbs_synth_rbsp_bound.argtypes = [C.c_uint64]
    lib.hbs_synth_rbsp_bound.restype = C.c_uint64
    lib.hbs_pair_alloc.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p), C.c_void_p]
    lib.hbs_pair_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.hbs_ctx_last_emit_by_tiles.argtypes = [C.c_void_p]
    lib.hbs_filter_annexb.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.hbs_access_units.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                     C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hbs_au_keep.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
    lib.hbs_au_sps_poc_offset.argtypes = []
    lib.hbs_annexb_to_lenpref.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.hbs_lenpref_to_annexb.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64,
                                          C.c_int, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.hbs_au_sps_poc_offset.restype = C.c_uint64
    lib.hbs_ts_demux.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                 C.c_void_p]
    lib.hbs_ts_packet_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.hbs_ts_find_pid_host.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.hbs_ts_mux.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.hbs_ts_mux_psi_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hbs_ts_mux_au_packets_host.argtypes = [C.c_uint64, C.c_int, C.c_int]
    lib.hbs_ts_mux_au_packets_host.restype = C.c_uint64
    lib.hbs_au_insert.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                  C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                  C.c_void_p, C.c_void_p]
    lib.hbs_aud_nal_host.argtypes = [C.c_int, C.c_uint32, C.c_void_p]
    lib.hbs_rtp_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hbs_rtp_nal_packets_host.argtypes = [C.c_uint64, C.c_int]
    lib.hbs_rtp_nal_packets_host.restype = C.c_uint64
    lib.hbs_rtp_packet_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.hbs_rtp_ap_units_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
    lib.hbs_rtp_ap_units_host.restype = C.c_int64
    lib.hbs_rtp_unpack.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                   C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.hbs_rtp_frames_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.hbs_rtp_frames_host.restype = C.c_uint64
    lib.hbs_rtp_order.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.hbs_au_times.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hbs_au_times.restype = C.c_int
    lib.hbs_cenc_subsamples.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.hbs_cenc_subsamples.restype = C.c_int
    lib.hbs_cenc_crypt.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]
    lib.hbs_cenc_crypt.restype = C.c_int
    lib.hbs_cbcs_crypt.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]
    lib.hbs_cbcs_crypt.restype = C.c_int
    lib.hbs_mp4_fragment.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                     C.c_void_p]
    lib.hbs_mp4_fragment_bytes_host.argtypes = [C.c_uint64, C.c_uint64]
    lib.hbs_mp4_fragment_bytes_host.restype = C.c_uint64
    lib.hbs_mp4_init_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.hbs_mp4_init_host.restype = C.c_int64
    lib.hbs_mp4_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hbs_mp4_samples.restype = C.c_int
    lib.hbs_mp4_init_read_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    lib.hbs_mp4_init_read_host.restype = C.c_int64
    lib.hbs_mp4_track_read_host.argtypes = lib.hbs_mp4_init_read_host.argtypes
    lib.hbs_mp4_track_read_host.restype = C.c_int64
    lib.hbs_mp4_stbl_find_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]
    lib.hbs_mp4_stbl_find_host.restype = C.c_int
    lib.hbs_mp4_stbl_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
    lib.hbs_mp4_stbl_samples.restype = C.c_int
    lib.hbs_mp4_stbl_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_uint64, C.c_void_p, C.c_void_p]
    lib.hbs_mp4_stbl_write.restype = C.c_int
    lib.hbs_mp4_stbl_write_bytes_host.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_uint32]
    lib.hbs_mp4_stbl_write_bytes_host.restype = C.c_uint64
    lib.hbs_mp4_moov_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.hbs_mp4_moov_host.restype = C.c_int64
    lib.hbs_mp4_protect.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                    C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hbs_mp4_protect.restype = C.c_int
    lib.hbs_mp4_protect_bytes_host.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    lib.hbs_mp4_protect_bytes_host.restype = C.c_uint64
    lib.hbs_mp4_init_protect_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                              C.c_uint64]
    lib.hbs_mp4_init_protect_host.restype = C.c_int64
    lib.hbs_mp4_senc_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.hbs_mp4_senc_samples.restype = C.c_int
    lib.hbs_mp4_init_unprotect_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                C.c_void_p, C.c_void_p, C.c_uint64]
    lib.hbs_mp4_init_unprotect_host.restype = C.c_int64
    _lib = lib
    return lib


def ts_packet(packet, pid, packet_bytes=188):
    """hbs_ts_packet_host: the packet rule of hbs_ts_demux for one packet (bytes or a uint8 array of packet_bytes bytes) in host
    memory -> a TS_PACKET record.  No GPU involved."""
    a = np.ascontiguousarray(np.frombuffer(bytes(packet), dtype=np.uint8) if isinstance(packet, (bytes, bytearray)) else packet, dtype=np.uint8)
    if len(a) != packet_bytes:
        raise HbsError("hbs_ts_packet_host: %d bytes given, packets are %d" % (len(a), packet_bytes))
    out = np.zeros(1, dtype=TS_PACKET)
    rc = load_library().hbs_ts_packet_host(a.ctypes.data, int(packet_bytes), int(pid), out.ctypes.data)
    if rc != 0:
        raise HbsError("hbs_ts_packet_host failed: %d" % rc)
    return out[0]


def ts_find_pid(head, packet_bytes=188, stream_type=STREAM_TYPE_HEVC):
    """hbs_ts_find_pid_host: (PID, program number) of the first elementary stream of `stream_type` in the first program of the
    transport stream whose first bytes are `head` (bytes or a uint8 array, host memory), or None.  No GPU involved."""
    a = np.ascontiguousarray(np.frombuffer(bytes(head), dtype=np.uint8) if isinstance(head, (bytes, bytearray)) else head, dtype=np.uint8)
    prog = C.c_int(0)
    pid = load_library().hbs_ts_find_pid_host(a.ctypes.data if len(a) else None, len(a), int(packet_bytes), int(stream_type), C.byref(prog))
    return None if pid < 0 else (pid, prog.value)


def ts_mux_params(pid=0x100, pmt_pid=0x1000, packet_bytes=188, program_number=1, transport_stream_id=1, flags=0,
                  cc_es=0, cc_pat=0, cc_pmt=0, pcr_lead=0, reserved=0):
    """an hbs_ts_mux_params record (ndarray[TS_MUX_PARAMS] of one, host memory)"""
    p = np.zeros(1, dtype=TS_MUX_PARAMS)
    p[0] = (packet_bytes, pid, pmt_pid, program_number, transport_stream_id, flags, cc_es, cc_pat, cc_pmt, reserved, pcr_lead)
    return p


def ts_mux_psi(params=None, **kw):
    """hbs_ts_mux_psi_host: the PAT and the PMT packet (188 bytes each) hbs_ts_mux places in front of AU 0, for an
    ndarray[TS_MUX_PARAMS] of one or the keywords of ts_mux_params.  No GPU involved."""
    p = np.ascontiguousarray(params, dtype=TS_MUX_PARAMS) if params is not None else ts_mux_params(**kw)
    pat, pmt = np.zeros(188, dtype=np.uint8), np.zeros(188, dtype=np.uint8)
    rc = load_library().hbs_ts_mux_psi_host(p.ctypes.data, pat.ctypes.data, pmt.ctypes.data)
    if rc != 0:
        raise HbsError("hbs_ts_mux_psi_host failed: %d" % rc)
    return pat.tobytes(), pmt.tobytes()


def ts_mux_au_packets(es_bytes, time_fields=0, pcr=False):
    """hbs_ts_mux_au_packets_host: the transport packets of an access unit of es_bytes bytes; time_fields 0: no time, 1: a PTS,
    2: a PTS and a DTS that differs.  No GPU involved."""
    return int(load_library().hbs_ts_mux_au_packets_host(int(es_bytes), int(time_fields), 1 if pcr else 0))


def aud_nal(temporal_id_plus1, slice_types):
    """hbs_aud_nal_host: the seven bytes (start code included) of the access-unit delimiter hbs_au_insert places in front of an
    AU whose record has that temporal_id_plus1 and slice_types.  No GPU involved."""
    out = np.zeros(7, dtype=np.uint8)
    rc = load_library().hbs_aud_nal_host(int(temporal_id_plus1), int(slice_types) & 0xFFFFFFFF, out.ctypes.data)
    if rc != 0:
        raise HbsError("hbs_aud_nal_host failed: %d" % rc)
    return out.tobytes()


def rtp_params(max_payload=1188, payload_type=96, framing=0, flags=0, ssrc=0, seq=0, ts_base=0, ts_step=0):
    """an hbs_rtp_params record (ndarray[RTP_PARAMS] of one, host memory)"""
    p = np.zeros(1, dtype=RTP_PARAMS)
    p[0] = (max_payload, payload_type, framing, flags, ssrc, seq, ts_base, ts_step)
    return p


def rtp_nal_packets(nal_bytes, max_payload):
    """hbs_rtp_nal_packets_host: the RTP packets of a NAL of nal_bytes bytes (0: below 2 bytes, or a max_payload out of range).
    No GPU involved."""
    return int(load_library().hbs_rtp_nal_packets_host(int(nal_bytes), int(max_payload)))


def rtp_packet(packet):
    """hbs_rtp_packet_host: one RTP packet (bytes or a uint8 array, without a length field, host memory) as a receiver reads it
    -> an RTP_PACKET record.  No GPU involved."""
    a = np.ascontiguousarray(np.frombuffer(bytes(packet), dtype=np.uint8) if isinstance(packet, (bytes, bytearray)) else packet, dtype=np.uint8)
    out = np.zeros(1, dtype=RTP_PACKET)
    rc = load_library().hbs_rtp_packet_host(a.ctypes.data if len(a) else None, len(a), out.ctypes.data)
    if rc != 0:
        raise HbsError("hbs_rtp_packet_host failed: %d" % rc)
    return out[0]


def rtp_ap_units(packet):
    """hbs_rtp_ap_units_host: the NAL units of one aggregation packet (bytes or a uint8 array, without a length field, host
    memory) -> (offsets within the packet ndarray[uint64], sizes ndarray[uint64]).  Raises HbsError for a packet that is no
    well-formed aggregation packet.  No GPU involved."""
    a = np.ascontiguousarray(np.frombuffer(bytes(packet), dtype=np.uint8) if isinstance(packet, (bytes, bytearray)) else packet, dtype=np.uint8)
    lib = load_library()
    ptr = a.ctypes.data if len(a) else None
    units = int(lib.hbs_rtp_ap_units_host(ptr, len(a), None, None, 0))
    if units < 0:
        raise HbsError("hbs_rtp_ap_units_host failed: %d" % units)
    off, size = np.zeros(units, dtype=np.uint64), np.zeros(units, dtype=np.uint64)
    lib.hbs_rtp_ap_units_host(ptr, len(a), off.ctypes.data, size.ctypes.data, units)
    return off, size


def rtp_packet_offsets(nal_off, nal_packet, max_payload, framing=0):
    """the output offset of every packet of an hbs_rtp_pack call, and the total behind them (packets + 1 entries), from the two
    per-NAL tables: all packets of a NAL but its last take framing + 12 + max_payload bytes.  With RTP_AGGREGATE the units of an
    aggregation packet share a packet number: NAL k opens a packet when k == 0 or nal_packet[k] != nal_packet[k - 1]"""
    nal_off, nal_packet = np.asarray(nal_off, dtype=np.uint64), np.asarray(nal_packet, dtype=np.uint64)
    opens = np.concatenate([[True], nal_packet[1:-1] != nal_packet[:-2]]) if len(nal_packet) > 1 else np.zeros(0, dtype=bool)
    begin, number = nal_off[:-1][opens], nal_packet[:-1][opens]
    count = np.diff(np.concatenate([number, nal_packet[-1:]])).astype(np.int64)
    first = np.repeat(number, count)
    within = np.arange(int(nal_packet[-1]), dtype=np.uint64) - first
    off = np.repeat(begin, count) + within * np.uint64(int(framing) + 12 + int(max_payload))
    return np.concatenate([off, nal_off[-1:]]).astype(np.uint64)


def rtp_unpack_params(payload_type=96, startcode_bytes=4, flags=0, ssrc=0):
    """an hbs_rtp_unpack_params record (ndarray[RTP_UNPACK_PARAMS] of one, host memory)"""
    p = np.zeros(1, dtype=RTP_UNPACK_PARAMS)
    p[0] = (payload_type, startcode_bytes, flags, ssrc)
    return p


def rtp_order_params(payload_type=96, flags=0, ssrc=0, max_span=1 << 20, after_ext=0):
    """an hbs_rtp_order_params record (ndarray[RTP_ORDER_PARAMS] of one, host memory)"""
    p = np.zeros(1, dtype=RTP_ORDER_PARAMS)
    p[0] = (payload_type, flags, ssrc, 0, max_span, after_ext)
    return p


def au_times_params(tick=1, base_time=0, delay=None, flags=0):
    """an hbs_au_times_params record (ndarray[AU_TIMES_PARAMS] of one, host memory); a delay sets HBS_AUT_DELAY_GIVEN"""
    p = np.zeros(1, dtype=AU_TIMES_PARAMS)
    p["flags"], p["tick"], p["base_time"] = flags | (AUT_DELAY_GIVEN if delay is not None else 0), tick, base_time
    p["delay"] = 0 if delay is None else delay
    return p


def cenc_plan_params(length_size=4, flags=0, clear_lead=96):
    """an hbs_cenc_plan_params record (ndarray[CENC_PLAN_PARAMS] of one, host memory)"""
    p = np.zeros(1, dtype=CENC_PLAN_PARAMS)
    p[0] = (length_size, flags, clear_lead, 0)
    return p


def cenc_params(key, iv0=None, iv_mode=None, scheme=CENC_SCHEME_CENC):
    """an hbs_cenc_params record (ndarray[CENC_PARAMS] of one, host memory).  key: 16 bytes; iv0: None, or 8 or 16 bytes (the
    first 8 count), which sets iv_mode 1 unless iv_mode says otherwise"""
    p = np.zeros(1, dtype=CENC_PARAMS)
    p["key"][0] = np.frombuffer(bytes(key), dtype=np.uint8)
    if iv0 is not None:
        b = bytes(iv0)
        p["iv0"][0][: len(b)] = np.frombuffer(b, dtype=np.uint8)
    p["scheme"], p["iv_mode"] = scheme, (0 if iv0 is None else 1) if iv_mode is None else iv_mode
    return p


def cbcs_params(key, iv0=None, iv_mode=None, flags=0, crypt_byte_block=1, skip_byte_block=9):
    """an hbs_cbcs_params record (ndarray[CBCS_PARAMS] of one, host memory).  key: 16 bytes; iv0: None, or the 16-byte constant
    IV, which sets iv_mode 1 unless iv_mode says otherwise; flags: CBCS_DECRYPT | CBCS_WHOLE_RUNS"""
    p = np.zeros(1, dtype=CBCS_PARAMS)
    p["key"][0] = np.frombuffer(bytes(key), dtype=np.uint8)
    if iv0 is not None:
        b = bytes(iv0)
        p["iv0"][0][: len(b)] = np.frombuffer(b, dtype=np.uint8)
    p["iv_mode"], p["flags"] = (0 if iv0 is None else 1) if iv_mode is None else iv_mode, flags
    p["crypt_byte_block"], p["skip_byte_block"] = crypt_byte_block, skip_byte_block
    return p


def mp4_params(length_size=4, flags=0, track_id=1, sequence=1, max_samples=0, sample_duration=0, base_time=0):
    """an hbs_mp4_params record (ndarray[MP4_PARAMS] of one, host memory)"""
    p = np.zeros(1, dtype=MP4_PARAMS)
    p[0] = (length_size, flags, track_id, sequence, max_samples, sample_duration, base_time)
    return p


def mp4_fragment_bytes(samples, sample_bytes):
    """hbs_mp4_fragment_bytes_host: the bytes of one fragment of `samples` samples that hold `sample_bytes` bytes"""
    return int(load_library().hbs_mp4_fragment_bytes_host(int(samples), int(sample_bytes)))


def mp4_init(nals, track_id=1, timescale=90000, width=1920, height=1080, length_size=4, chroma_format_idc=1, bit_depth_luma=8,
             bit_depth_chroma=8, flags=0, _moov=None):
    """hbs_mp4_init_host: the init segment (ftyp + moov) for the fragments of hbs_mp4_fragment, as bytes.  nals: the VPS / SPS /
    PPS NAL units (bytes-like, no start codes), in the order their arrays list them.  Raises HbsError for what the call refuses."""
    lib = load_library()
    name = "hbs_mp4_moov_host" if _moov is not None else "hbs_mp4_init_host"
    call = getattr(lib, name)
    prm = np.zeros(1, dtype=MP4_INIT_PARAMS)
    prm[0] = (track_id, timescale, width, height, length_size, chroma_format_idc, bit_depth_luma, bit_depth_chroma)
    bufs = [np.frombuffer(bytes(x), dtype=np.uint8) if len(x) else np.zeros(0, dtype=np.uint8) for x in nals]
    ptrs = (C.c_void_p * max(len(bufs), 1))(*[b.ctypes.data if b.size else None for b in bufs])
    sizes = np.array([b.size for b in bufs], dtype=np.uint64)
    args = (prm.ctypes.data_as(C.c_void_p), int(flags), C.cast(ptrs, C.c_void_p), sizes.ctypes.data_as(C.c_void_p), len(bufs))
    if _moov is not None:
        args += (int(_moov[0]), int(_moov[1]))
    need = int(call(*args, None, 0))
    if need < 0:
        raise HbsError("%s: error %d" % (name, need))
    out = np.zeros(need, dtype=np.uint8)
    got = int(call(*args, out.ctypes.data_as(C.c_void_p), need))
    if got != need:
        raise HbsError("%s: %d, then %d" % (name, need, got))
    return out.tobytes()


def mp4_moov(nals, duration, tables_bytes, **kw):
    """hbs_mp4_moov_host: ftyp and the moov of a progressive file up to and including the stsd, as bytes; the `tables_bytes` bytes
    that hbs_mp4_stbl_write writes complete the moov.  duration: reserved[1] of that call's summary.  The other arguments are
    mp4_init's.  Raises HbsError for what the call refuses."""
    return mp4_init(nals, _moov=(duration, tables_bytes), **kw)


def mp4_protect_params(iv_size=8, flags=0):
    """an hbs_mp4_protect_params record (ndarray[MP4_PROTECT_PARAMS] of one, host memory)"""
    p = np.zeros(1, dtype=MP4_PROTECT_PARAMS)
    p["iv_size"], p["flags"] = iv_size, flags
    return p


def mp4_protect_bytes(samples, entries, iv_size):
    """hbs_mp4_protect_bytes_host: the bytes a fragment of `samples` samples with `entries` subsample entries grows by"""
    return int(load_library().hbs_mp4_protect_bytes_host(int(samples), int(entries), int(iv_size)))


def mp4_init_protect(init_bytes, kid, scheme=MP4_SCHEME_CENC, iv_size=8, constant_iv=None, crypt_byte_block=0, skip_byte_block=0,
                     pssh=(), track_id=0, tenc=None):
    """hbs_mp4_init_protect_host: the init segment (bytes-like) with the track's sample entry turned into 'encv' with sinf /
    frma / schm / schi / tenc, and the given whole 'pssh' boxes (bytes-like each) appended to the moov, as bytes.  kid: 16
    bytes; constant_iv: None, or 8 or 16 bytes with iv_size 0; tenc: an ndarray[MP4_TENC] of one in place of those keywords.
    Raises HbsError for what the call refuses."""
    lib = load_library()
    if tenc is None:
        tenc = np.zeros(1, dtype=MP4_TENC)
        tenc["scheme"], tenc["crypt_byte_block"], tenc["skip_byte_block"], tenc["iv_size"] = scheme, crypt_byte_block, skip_byte_block, iv_size
        tenc["kid"][0] = np.frombuffer(bytes(kid), dtype=np.uint8)
        if constant_iv is not None:
            b = bytes(constant_iv)
            tenc["constant_iv_size"] = len(b)
            tenc["constant_iv"][0][: len(b)] = np.frombuffer(b, dtype=np.uint8)
    tenc, tenc_p = _rec(tenc, MP4_TENC)
    seg = np.frombuffer(bytes(init_bytes), dtype=np.uint8)
    bufs = [np.frombuffer(bytes(x), dtype=np.uint8) if len(x) else np.zeros(0, dtype=np.uint8) for x in pssh]
    ptrs = (C.c_void_p * max(len(bufs), 1))(*[b.ctypes.data if b.size else None for b in bufs])
    sizes = np.array([b.size for b in bufs], dtype=np.uint64)
    args = (seg.ctypes.data_as(C.c_void_p) if seg.size else None, seg.size, int(track_id), tenc_p, C.cast(ptrs, C.c_void_p),
            sizes.ctypes.data_as(C.c_void_p), len(bufs))
    need = int(lib.hbs_mp4_init_protect_host(*args, None, 0))
    if need < 0:
        raise HbsError("hbs_mp4_init_protect_host: error %d" % need)
    out = np.zeros(need, dtype=np.uint8)
    got = int(lib.hbs_mp4_init_protect_host(*args, out.ctypes.data_as(C.c_void_p), need))
    if got != need:
        raise HbsError("hbs_mp4_init_protect_host: %d, then %d" % (need, got))
    return out.tobytes()


def mp4_senc_params(iv_size=8, track_id=0, flags=0):
    """an hbs_mp4_senc_params record (ndarray[MP4_SENC_PARAMS] of one, host memory)"""
    p = np.zeros(1, dtype=MP4_SENC_PARAMS)
    p["iv_size"], p["track_id"], p["flags"] = iv_size, track_id, flags
    return p


def mp4_init_unprotect(init_bytes, track_id=0):
    """hbs_mp4_init_unprotect_host: the clear init segment of a protected one (bytes-like), with what its sinf and pssh boxes
    said.  Returns (bytes, tenc ndarray[MP4_TENC] of one, the frma fourcc as an int, [the whole 'pssh' boxes as bytes]).
    Raises HbsError for what the call refuses."""
    lib = load_library()
    seg = np.frombuffer(bytes(init_bytes), dtype=np.uint8)
    tenc = np.zeros(1, dtype=MP4_TENC)
    fmt, n_pssh = C.c_uint32(0), C.c_uint64(0)
    head = (seg.ctypes.data_as(C.c_void_p) if seg.size else None, seg.size, int(track_id), tenc.ctypes.data_as(C.c_void_p), C.byref(fmt))
    need = int(lib.hbs_mp4_init_unprotect_host(*head, None, None, 0, C.byref(n_pssh), None, 0))
    if need < 0:
        raise HbsError("hbs_mp4_init_unprotect_host: error %d" % need)
    k = int(n_pssh.value)
    off, size = np.zeros(max(k, 1), dtype=np.uint64), np.zeros(max(k, 1), dtype=np.uint64)
    out = np.zeros(max(need, 1), dtype=np.uint8)
    got = int(lib.hbs_mp4_init_unprotect_host(*head, off.ctypes.data_as(C.c_void_p), size.ctypes.data_as(C.c_void_p), k, C.byref(n_pssh),
                                              out.ctypes.data_as(C.c_void_p), need))
    if got != need or int(n_pssh.value) != k:
        raise HbsError("hbs_mp4_init_unprotect_host: %d, then %d" % (need, got))
    raw = seg.tobytes()
    return out[:need].tobytes(), tenc, int(fmt.value), [raw[int(o):int(o) + int(z)] for o, z in zip(off[:k], size[:k])]


def mp4_stbl_write_params(flags=0, max_chunk_samples=0, sample_duration=0, base_time=0, data_offset=0):
    """an hbs_mp4_stbl_write_params record (ndarray[MP4_STBL_WRITE_PARAMS] of one, host memory)"""
    p = np.zeros(1, dtype=MP4_STBL_WRITE_PARAMS)
    p[0] = (flags, max_chunk_samples, sample_duration, 0, base_time, data_offset)
    return p


def mp4_stbl_write_bytes(n_samples, with_ctts=True, with_stss=True, flags=0):
    """hbs_mp4_stbl_write_bytes_host: an upper bound of the bytes hbs_mp4_stbl_write writes for n_samples samples"""
    return int(load_library().hbs_mp4_stbl_write_bytes_host(int(n_samples), int(bool(with_ctts)), int(bool(with_stss)), int(flags)))


def mp4_read_params(track_id=0, trex_duration=0, trex_size=0, trex_flags=0, flags=0):
    """an hbs_mp4_read_params record (ndarray[MP4_READ_PARAMS] of one, host memory)"""
    p = np.zeros(1, dtype=MP4_READ_PARAMS)
    p[0] = (flags, track_id, trex_duration, trex_size, trex_flags, (0, 0, 0))
    return p


def mp4_init_read(segment_bytes, track_id=0, _call="hbs_mp4_init_read_host"):
    """hbs_mp4_init_read_host: the track record (an MP4_TRACK record) of an init segment (bytes-like) and the parameter-set NALs
    of its hvcC as slices of the segment, in array order.  Raises HbsError for what the call refuses."""
    lib = load_library()
    read = getattr(lib, _call)
    seg = np.frombuffer(bytes(segment_bytes), dtype=np.uint8)
    trk = np.zeros(1, dtype=MP4_TRACK)
    sp = seg.ctypes.data_as(C.c_void_p) if seg.size else None
    n = int(read(sp, seg.size, int(track_id), trk.ctypes.data_as(C.c_void_p), None, None, 0))
    if n < 0:
        raise HbsError("%s: error %d" % (_call, n))
    off, size = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
    got = int(read(sp, seg.size, int(track_id), trk.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                                         size.ctypes.data_as(C.c_void_p), n))
    if got != n:
        raise HbsError("%s: %d, then %d" % (_call, n, got))
    raw = seg.tobytes()
    return trk[0].copy(), [raw[int(off[i]): int(off[i]) + int(size[i])] for i in range(n)]


def mp4_track_read(file_bytes, track_id=0):
    """hbs_mp4_track_read_host: mp4_init_read for a progressive file (or its moov), which has no mvex: the same record with
    the trex fields 0, and the parameter-set NALs of the hvcC."""
    return mp4_init_read(file_bytes, track_id, _call="hbs_mp4_track_read_host")


def mp4_stbl_find(data, base=0, track_id=0):
    """hbs_mp4_stbl_find_host: where the sample table boxes of one track of a progressive MP4 lie (an ndarray[MP4_STBL] of one,
    host memory).  data: the file, or its moov alone with base = the moov's position in the file (bytes-like).  Raises HbsError
    for what the call refuses."""
    lib = load_library()
    seg = np.frombuffer(bytes(data), dtype=np.uint8)
    rec = np.zeros(1, dtype=MP4_STBL)
    rc = int(lib.hbs_mp4_stbl_find_host(seg.ctypes.data_as(C.c_void_p) if seg.size else None, seg.size, int(base), int(track_id),
                                        rec.ctypes.data_as(C.c_void_p)))
    if rc != 0:
        raise HbsError("hbs_mp4_stbl_find_host: error %d" % rc)
    return rec


def rtp_frames(data, cap=None):
    """hbs_rtp_frames_host: the packets of an RFC 4571 byte stream (bytes or a uint8 array, host memory) -> (packet offsets,
    packet sizes, bytes the whole frames take); the tables are what hbs_rtp_unpack takes.  cap: fill no more than that many
    entries (the frames are still counted: see the fourth value).  -> (off ndarray[uint64], size ndarray[uint64], used, frames).
    No GPU involved."""
    a = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data, dtype=np.uint8)
    lib = load_library()
    used = C.c_uint64(0)
    ptr = a.ctypes.data if len(a) else None
    if cap is None:
        cap = int(lib.hbs_rtp_frames_host(ptr, len(a), None, None, 0, C.byref(used)))
    off, size = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
    frames = int(lib.hbs_rtp_frames_host(ptr, len(a), off.ctypes.data if cap else None, size.ctypes.data if cap else None, cap, C.byref(used)))
    filled = min(frames, cap)
    return off[:filled], size[:filled], int(used.value), frames


# ---- what the device-call wrappers share ("adding a device call") ---------------------------------------------------

def _p(x):
    """a device tensor, or None, as the pointer argument of a foreign call"""
    return C.c_void_p(x.data_ptr()) if x is not None else None


def _rec(params, dtype):
    """a host parameter record, or None -> (the record's array, its pointer argument).  The pointer is good while the array
    lives: the caller keeps both in locals until the foreign call has returned."""
    if params is None:
        return None, None
    a = np.ascontiguousarray(params, dtype=dtype)
    return a, a.ctypes.data_as(C.c_void_p)


def _holds(x, width=1):
    """what the tensor x holds, in records of `width` bytes (None holds nothing): the default of a capacity"""
    return x.numel() * x.element_size() // width if x is not None else 0


def _host(x, n, dtype):
    """the first n records of a device tensor of bytes as a host array of `dtype`"""
    return x[: n * np.dtype(dtype).itemsize].cpu().numpy().view(dtype).copy()


class Context:
    """One per GPU (per rank).  Device buffers are torch uint8 CUDA tensors; the
    library runs on torch's current stream so that ordering with torch ops is
    the stream order."""

    def __init__(self, device=0):
        import torch
        self.torch = torch
        self.lib = load_library()
        self.device = int(device)
        h = C.c_void_p()
        rc = self.lib.hbs_ctx_create(C.byref(h), self.device)
        if rc != 0:
            raise HbsError("hbs_ctx_create(device=%d) failed: %d (no gfx950 GPU? there is no CPU fallback)"
                           % (self.device, rc))
        self.h = h
        self._bind_stream()

    def _bind_stream(self):
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        self.lib.hbs_ctx_set_stream(self.h, C.c_void_p(s))

    def close(self):
        if getattr(self, "h", None):
            self.lib.hbs_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise HbsError("%s failed: %d (%s)" % (what, rc, self.lib.hbs_last_error(self.h).decode()))

    # ---- plan, allocate, run: what the convenience wrappers of the device calls share ----

    def _empty(self, nbytes):
        return self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.torch.device("cuda", self.device))

    def _zeros(self, nbytes=SUMMARY.itemsize):
        """zeroed device bytes: by default the summary a call is given"""
        return self.torch.zeros(nbytes, dtype=self.torch.uint8, device=self.torch.device("cuda", self.device))

    def _dv(self, x, dtype=None, empty=True):
        """an ndarray (of `dtype`; None: its bytes as they are) or a device tensor of its bytes -> (device tensor of the bytes,
        entries).  None stays None: the C calls read a null pointer as "absent".  A table of no entries becomes 16 zeroed
        bytes, so that the call still gets a pointer (empty=False: None)."""
        if x is None:
            return None, 0
        if not isinstance(x, np.ndarray):
            return x, _holds(x, np.dtype(dtype).itemsize if dtype is not None else 1)
        b = np.ascontiguousarray(x, dtype=dtype).view(np.uint8).reshape(-1)
        if not b.size:
            return (self._zeros(16) if empty else None), 0
        return self.torch.from_numpy(b.copy()).to(self.torch.device("cuda", self.device)), len(x)

    def _raise_on(self, name, s, where=""):
        """HbsError for a summary that reports an error.  where: what follows "<name>: error %d", with {0} {1} {2} for the
        entries reserved[0..2] name (each is 1 + the entry), or a function of the summary that gives that text"""
        if int(s["error"]) != 0:
            where = where(s) if callable(where) else where
            raise HbsError("%s: error %d%s" % (name, int(s["error"]), where.format(*[int(r) - 1 for r in s["reserved"]])))

    def _run(self, name, rc, summary, where=""):
        """behind an enqueue (a plan or a run): its return code checked, the summary read -> the summary record"""
        self._check(rc, name)
        s = self.read_summary(summary)
        self._raise_on(name, s, where)
        return s

    def set_sequential_parse(self, on=True):
        """parse batches NAL after NAL with ONE set of derived RPS tables, as the reference does (slow, exact on any input)"""
        self.lib.hbs_ctx_set_sequential_parse.argtypes = [C.c_void_p, C.c_int]
        self._check(self.lib.hbs_ctx_set_sequential_parse(self.h, 1 if on else 0), "hbs_ctx_set_sequential_parse")

    def set_emit_path(self, path=-1):
        """-1 = picked per call (default), 0 = the single-pass emit kernel by NALs, 1 = count / scan / emit, 2 = the single pass by
        arena tiles whenever the index allows it"""
        self.lib.hbs_ctx_set_emit_path.argtypes = [C.c_void_p, C.c_int]
        self._check(self.lib.hbs_ctx_set_emit_path(self.h, path), "hbs_ctx_set_emit_path")

    def set_kernel(self, variant):
        """0 = automatic (a density probe picks 4, 6, 2 or 5 on the device; the default), 2 = LDS-image
        scan/extract kernel, 4 = event-sparse one, 5 = index-only streaming one (with an arena it means 4),
        6 = event-sparse one with 24 rows a wavefront"""
        self._check(self.lib.hbs_ctx_set_kernel(self.h, variant), "hbs_ctx_set_kernel")

    def set_count_ahead(self, mode=1):
        """dense tiles counted ahead of kernel 4 and of emit_annexb's arena-tile kernel: 0 never, 1 on streams / arenas
        of 3 GiB and more (default), 2 always"""
        self.lib.hbs_ctx_set_count_ahead.argtypes = [C.c_void_p, C.c_int]     # (bound here: development libraries of earlier rounds load too)
        self._check(self.lib.hbs_ctx_set_count_ahead(self.h, mode), "hbs_ctx_set_count_ahead")

    def kernel(self):
        return self.lib.hbs_ctx_get_kernel(self.h)

    def last_kernel(self):
        """the kernel that ran the last index_extract (waits for it)"""
        return self.lib.hbs_ctx_last_kernel(self.h)

    def enable_timing(self, on=True):
        self._check(self.lib.hbs_ctx_enable_timing(self.h, 1 if on else 0), "hbs_ctx_enable_timing")

    def kernel_ms(self):
        """Duration of the last fused scan/extract kernel (HIP events on its own stream)."""
        ms = C.c_float()
        self._check(self.lib.hbs_ctx_kernel_ms(self.h, C.byref(ms)), "hbs_ctx_kernel_ms")
        return ms.value

    def reserve_workgroups(self, spare):
        """leave `spare` workgroup slots of the persistent scan kernels free (for RCCL's kernels beside the scan)"""
        self.lib.hbs_ctx_reserve_workgroups.argtypes = [C.c_void_p, C.c_int]
        self._check(self.lib.hbs_ctx_reserve_workgroups(self.h, int(spare)), "hbs_ctx_reserve_workgroups")

    def set_device_exclusive(self, on):
        """1: this context's calls are the only persistent kernels on the device while they run (first tiles by workgroup
        number); 0 (default): every tile by ticket -- safe with several contexts or processes on one device"""
        self.lib.hbs_ctx_set_device_exclusive.argtypes = [C.c_void_p, C.c_int]
        self._check(self.lib.hbs_ctx_set_device_exclusive(self.h, int(on)), "hbs_ctx_set_device_exclusive")
        self.exclusive = int(on)

    def device_bytes(self):
        """device memory the context itself holds (grow-only scratch; caller-owned buffers are not counted)"""
        self.lib.hbs_ctx_device_bytes.restype = C.c_uint64
        self.lib.hbs_ctx_device_bytes.argtypes = [C.c_void_p]
        return int(self.lib.hbs_ctx_device_bytes(self.h))

    def kernel_ms_back(self, back):
        """Duration of the timed call `back` calls ago (0 = the last one; the library keeps the last 64)."""
        ms = C.c_float()
        self._check(self.lib.hbs_ctx_kernel_ms_back(self.h, back, C.byref(ms)), "hbs_ctx_kernel_ms_back")
        return ms.value

    def grid(self):
        a, b = C.c_int(), C.c_int()
        self.lib.hbs_ctx_grid(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def pair_alloc(self, peer, nbytes):
        """hbs_pair_alloc: `nbytes` of device memory placed against the tensor `peer` (the buffer it will be written from /
        read into), as a uint8 torch tensor that frees the memory when it dies.  Returns (tensor, report dict).  The
        probe runs on the current torch stream; `peer`'s contents do not matter."""
        t = self.torch
        self._bind_stream()
        self.lib.hbs_pair_alloc.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p), C.c_void_p]
        self.lib.hbs_pair_free.argtypes = [C.c_void_p, C.c_void_p]
        rep = np.zeros(1, dtype=PAIR_REPORT)
        ptr = C.c_void_p()
        rc = self.lib.hbs_pair_alloc(self.h, C.c_void_p(peer.data_ptr()) if peer is not None else None,
                                     peer.numel() * peer.element_size() if peer is not None else 0, nbytes, C.byref(ptr), rep.ctypes.data)
        self._check(rc, "hbs_pair_alloc")
        holder = _PairedMemory(self.lib, ptr.value, nbytes)
        tensor = t.as_tensor(holder, device=t.device("cuda", self.device))       # zero-copy: torch keeps `holder` alive
        assert tensor.data_ptr() == ptr.value
        return tensor, {k: int(rep[0][k]) for k in PAIR_REPORT.names if k != "reserved"}

    def alloc_outputs(self, stream_bytes, index_cap=None, want_rbsp=True, peer=None):
        """Device buffers sized for a stream: (index[u8, cap*32], rbsp[u8] or None, summary[u8, 64]).
        peer: the stream tensor the arena will be written from -- the arena is then placed against it (pair_alloc:
        4-5 % on multi-GiB streams; self.last_pair_report says what the probe found)."""
        t = self.torch
        dev = t.device("cuda", self.device)
        if index_cap is None:
            index_cap = self.default_index_cap(stream_bytes)
        index = t.empty(max(index_cap, 1) * NAL_ENTRY.itemsize, dtype=t.uint8, device=dev)
        if want_rbsp and peer is not None:
            rbsp, self.last_pair_report = self.pair_alloc(peer, stream_bytes + 16)
        else:
            rbsp = t.empty(stream_bytes + 16, dtype=t.uint8, device=dev) if want_rbsp else None
        summary = t.zeros(SUMMARY.itemsize, dtype=t.uint8, device=dev)
        return index, rbsp, summary, index_cap

    @staticmethod
    def default_index_cap(stream_bytes):
        """Entries to provide when the caller does not say.  The worst case -- a start code every three bytes -- is
        stream_bytes / 3 entries of 32 bytes, ten times the stream, all of it cleared by every scan: fine for small
        streams (tests full of tiny NALs), ruinous for a 1 GiB one.  From 64 MiB on: one entry per 64 stream bytes (coded
        video has one per several KiB); a stream with more NALs than that reports HBS_E_CAPACITY in its summary and
        nal_found says how many entries it needs (index_extract() below then runs it again with that many)."""
        worst = stream_bytes // 3 + 2
        return worst if stream_bytes <= (64 << 20) else min(worst, stream_bytes // 64 + 4096)

    def index_extract_async(self, stream, index, index_cap, rbsp, summary):
        """Enqueue K12 on the current torch stream.  All arguments are device tensors.  A stream with more NALs than
        index_cap reports HBS_E_CAPACITY in its summary (nal_found = the entries it needs): alloc_outputs() defaults to
        default_index_cap(), which is NOT the worst case above 64 MiB -- index_extract() retries with a larger index,
        callers of this method do that themselves."""
        self._bind_stream()
        rc = self.lib.hbs_index_extract(self.h, C.c_void_p(stream.data_ptr() if stream.numel() else None),
                                        stream.numel(), C.c_void_p(index.data_ptr()), index_cap,
                                        C.c_void_p(rbsp.data_ptr()) if rbsp is not None else None,
                                        rbsp.numel() if rbsp is not None else 0,
                                        C.c_void_p(summary.data_ptr()))
        self._check(rc, "hbs_index_extract")

    def read_summary(self, summary):
        out = np.zeros(1, dtype=SUMMARY)
        rc = self.lib.hbs_read_summary(self.h, C.c_void_p(summary.data_ptr()), out.ctypes.data)
        self._check(rc, "hbs_read_summary")
        return out[0]

    def index_extract(self, stream, index_cap=None, want_rbsp=True):
        """Convenience: run K12 and bring the results to the host.
        Returns (entries ndarray[NAL_ENTRY], arena ndarray[u8] or None, summary record)."""
        index, rbsp, summary, cap = self.alloc_outputs(stream.numel(), index_cap, want_rbsp)
        self.index_extract_async(stream, index, cap, rbsp, summary)
        s = self.read_summary(summary)
        if index_cap is None and int(s["error"]) == -4 and int(s["nal_found"]) > cap:      # HBS_E_CAPACITY: the default was too small
            # only the index grows: the arena and the summary of the first attempt are used again (a second arena next to the
            # first would double the peak for exactly the large streams the reduced default is for)
            del index
            cap = int(s["nal_found"]) + 8
            index = self.torch.empty(cap * NAL_ENTRY.itemsize, dtype=self.torch.uint8, device=summary.device)
            summary.zero_()
            self.index_extract_async(stream, index, cap, rbsp, summary)
            s = self.read_summary(summary)
        n = int(s["nal_count"])
        ent = index[: n * NAL_ENTRY.itemsize].cpu().numpy().view(NAL_ENTRY).copy()
        arena = rbsp[: int(s["rbsp_bytes"])].cpu().numpy() if want_rbsp else None
        return ent, arena, s

    # ---- K3 and the synthetic workload -------------------------------------------------

    def set_ingest_window_max(self, max_bytes):
        """ceiling of the window growth of index_extract_host (a NAL longer than the window doubles it); 0: the default, 1 GiB"""
        self.lib.hbs_ctx_set_ingest_window_max.argtypes = [C.c_void_p, C.c_uint64]
        self._check(self.lib.hbs_ctx_set_ingest_window_max(self.h, int(max_bytes)), "hbs_ctx_set_ingest_window_max")

    def index_extract_host(self, stream, window_bytes=256 << 20, index_cap=None, want_rbsp=True, pinned=True):
        """Windowed ingest of a HOST stream of any length (hbs_index_extract_host): `stream` is a numpy
        uint8 array (or anything np.asarray accepts).  Returns (entries ndarray[NAL_ENTRY], arena ndarray
        or None, summary record).  pinned=True stages the stream and the outputs in page-locked memory so
        that uploads, scans and downloads overlap."""
        t = self.torch
        a = np.ascontiguousarray(np.asarray(stream, dtype=np.uint8))
        n = int(a.size)
        cap = (n // 3 + 2) if index_cap is None else int(index_cap)

        def host(nbytes):
            buf = t.empty(max(nbytes, 16), dtype=t.uint8)
            return buf.pin_memory() if pinned else buf
        h_stream = host(n)
        if n:
            h_stream[:n].copy_(t.from_numpy(a))
        h_index = host(max(cap, 1) * NAL_ENTRY.itemsize)
        h_rbsp = host(n + 16) if want_rbsp else None
        summ = np.zeros(1, dtype=SUMMARY)
        rc = self.lib.hbs_index_extract_host(self.h, C.c_void_p(h_stream.data_ptr()), n, int(window_bytes),
                                             C.c_void_p(h_index.data_ptr()), cap,
                                             C.c_void_p(h_rbsp.data_ptr()) if h_rbsp is not None else None, n + 16,
                                             summ.ctypes.data_as(C.c_void_p))
        self._check(rc, "hbs_index_extract_host")
        s = summ[0]
        cnt = int(s["nal_count"])
        ent = h_index.numpy()[: cnt * NAL_ENTRY.itemsize].view(NAL_ENTRY).copy()
        arena = h_rbsp.numpy()[: int(s["rbsp_bytes"])].copy() if h_rbsp is not None else None
        return ent, arena, s

    def write_headers(self, parsed, structs, n_nals, rbsp_cap):
        """K5: serialise the structs of a parsed batch back to RBSP.  parsed: ndarray[PARSED] (host) or a device
        uint8 tensor of n records; structs: the device struct arena hbs_parse_headers filled.  Returns
        (written ndarray[WRITTEN], rbsp device tensor of n_nals * rbsp_cap bytes)."""
        t = self.torch
        dev = t.device("cuda", self.device)
        if isinstance(parsed, np.ndarray):
            parsed = t.from_numpy(np.ascontiguousarray(parsed).view(np.uint8).copy()).to(dev)
        out = t.empty(max(n_nals, 1) * rbsp_cap, dtype=t.uint8, device=dev)
        written = t.empty(max(n_nals, 1) * WRITTEN.itemsize, dtype=t.uint8, device=dev)
        self._bind_stream()
        rc = self.lib.hbs_write_headers(self.h, C.c_void_p(parsed.data_ptr()), n_nals, C.c_void_p(structs.data_ptr()),
                                        None, None, C.c_void_p(out.data_ptr()), rbsp_cap, C.c_void_p(written.data_ptr()))
        self._check(rc, "hbs_write_headers")
        return written[: n_nals * WRITTEN.itemsize].cpu().numpy().view(WRITTEN).copy(), out

    def emit_annexb_async(self, rbsp, rbsp_bytes, index, n_nals, gap_mode, out, index_out, summary):
        """Enqueue K3.  rbsp/index/out/index_out/summary are device tensors (index_out may be None)."""
        self._bind_stream()
        rc = self.lib.hbs_emit_annexb(self.h, C.c_void_p(rbsp.data_ptr()), rbsp_bytes, C.c_void_p(index.data_ptr()),
                                      n_nals, gap_mode, C.c_void_p(out.data_ptr()), out.numel(),
                                      C.c_void_p(index_out.data_ptr()) if index_out is not None else None,
                                      C.c_void_p(summary.data_ptr()))
        self._check(rc, "hbs_emit_annexb")

    def emit_annexb(self, rbsp, index_entries, gap_mode=0, out_cap=None):
        """Convenience: entries is a host ndarray[NAL_ENTRY]; returns (stream ndarray, entries_out).
        out_cap: size of the output buffer (default: the bound that always fits)."""
        t = self.torch
        dev = t.device("cuda", self.device)
        n = len(index_entries)
        d_idx = t.from_numpy(np.ascontiguousarray(index_entries).view(np.uint8).copy()).to(dev) if n else \
            t.zeros(NAL_ENTRY.itemsize, dtype=t.uint8, device=dev)
        rbsp_bytes = int(rbsp.numel())
        if out_cap is None:
            if gap_mode == 0 and n:          # the recorded gaps come on top of the 3/2 bound
                e = index_entries
                gaps = int(e["start"][0]) + int((e["start"][1:].astype(np.int64) - e["end"][:-1].astype(np.int64)).clip(min=0).sum())
                self.lib.hbs_annexb_bound_gaps.restype = C.c_uint64
                self.lib.hbs_annexb_bound_gaps.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
                out_cap = int(self.lib.hbs_annexb_bound_gaps(rbsp_bytes, n, gaps)) + 64
            else:
                out_cap = int(self.lib.hbs_annexb_bound(rbsp_bytes, n)) + 64
        out = t.empty(out_cap, dtype=t.uint8, device=dev)
        d_out_idx = t.empty(max(n, 1) * NAL_ENTRY.itemsize, dtype=t.uint8, device=dev)
        summary = t.zeros(SUMMARY.itemsize, dtype=t.uint8, device=dev)
        if rbsp_bytes == 0:
            rbsp = t.zeros(16, dtype=t.uint8, device=dev)
        self.emit_annexb_async(rbsp, rbsp_bytes, d_idx, n, gap_mode, out, d_out_idx, summary)
        s = self.read_summary(summary)
        if int(s["error"]) != 0:
            raise HbsError("hbs_emit_annexb: error %d" % int(s["error"]))
        return (out[: int(s["stream_bytes"])].cpu().numpy(),
                d_out_idx[: n * NAL_ENTRY.itemsize].cpu().numpy().view(NAL_ENTRY).copy())

    def synth_stream(self, seed, n_nals, mode=0):
        """Generate S(seed, n_nals, mode) in HBM.  Returns device tensors and sizes:
        dict(stream=u8[stream_bytes...], stream_bytes, rbsp=u8[...], rbsp_bytes, index=u8[n*32])."""
        t = self.torch
        dev = t.device("cuda", self.device)
        rbsp_cap = int(self.lib.hbs_synth_rbsp_bound(n_nals))
        rbsp = t.empty(rbsp_cap, dtype=t.uint8, device=dev)
        index = t.empty(max(n_nals, 1) * NAL_ENTRY.itemsize, dtype=t.uint8, device=dev)
        summary = t.zeros(SUMMARY.itemsize, dtype=t.uint8, device=dev)
        self._bind_stream()
        rc = self.lib.hbs_synth_rbsp(self.h, seed, n_nals, mode, C.c_void_p(rbsp.data_ptr()), rbsp_cap,
                                     C.c_void_p(index.data_ptr()), C.c_void_p(summary.data_ptr()))
        self._check(rc, "hbs_synth_rbsp")
        s = self.read_summary(summary)
        if int(s["error"]) != 0:
            raise HbsError("hbs_synth_rbsp: error %d" % int(s["error"]))
        rbsp_bytes = int(s["stream_bytes"])
        out_cap = int(self.lib.hbs_annexb_bound(rbsp_bytes, n_nals))
        stream = t.empty(out_cap, dtype=t.uint8, device=dev)
        self.emit_annexb_async(rbsp, rbsp_bytes, index, n_nals, 1, stream, index, summary)
        s = self.read_summary(summary)
        if int(s["error"]) != 0:
            raise HbsError("hbs_emit_annexb: error %d" % int(s["error"]))
        return dict(stream=stream, stream_bytes=int(s["stream_bytes"]), rbsp=rbsp, rbsp_bytes=rbsp_bytes,
                    index=index, n_nals=n_nals)

    # ---- K4 ---------------------------------------------------------------------------

    def parse_headers_async(self, rbsp, index, n_nals, parsed, structs, summary):
        """Enqueue K4.  All arguments are device tensors; structs may be None (plan only)."""
        self._bind_stream()
        rc = self.lib.hbs_parse_headers(self.h, C.c_void_p(rbsp.data_ptr()), C.c_void_p(index.data_ptr()), n_nals,
                                        C.c_void_p(parsed.data_ptr()),
                                        C.c_void_p(structs.data_ptr()) if structs is not None else None,
                                        structs.numel() if structs is not None else 0, C.c_void_p(summary.data_ptr()))
        self._check(rc, "hbs_parse_headers")

    def index_parse_async(self, stream, index, index_cap, parsed, structs, scan_summary, parse_summary, window=0, payload_off=None):
        """hbs_index_parse: index-only scan + header parse without an RBSP arena.  All arguments are device tensors
        (structs may be None: plan only; payload_off: optional int64 tensor, one per index entry).  Returns the NAL count
        (the call waits for the scan; the parse is enqueued behind it)."""
        self._bind_stream()
        self.lib.hbs_index_parse.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                             C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        n = C.c_uint64(0)
        rc = self.lib.hbs_index_parse(self.h, C.c_void_p(stream.data_ptr() if stream.numel() else None), stream.numel(),
                                      C.c_void_p(index.data_ptr()), index_cap, window, C.c_void_p(parsed.data_ptr()),
                                      C.c_void_p(structs.data_ptr()) if structs is not None else None,
                                      structs.numel() if structs is not None else 0,
                                      C.c_void_p(payload_off.data_ptr()) if payload_off is not None else None,
                                      C.c_void_p(scan_summary.data_ptr()), C.c_void_p(parse_summary.data_ptr()), C.byref(n))
        self._check(rc, "hbs_index_parse")
        return int(n.value)

    def parse_compact_async(self, rbsp, index, n_nals, parsed, compact, structs, summary, want=None, initial_sps_slot=None, initial_pps=None):
        """hbs_parse_headers_compact (want is None) / hbs_parse_materialize (want: int64 / uint64 device tensor of NAL numbers).
        structs None: plan only."""
        self._bind_stream()
        p = _p
        common = [self.h, p(rbsp), p(index), n_nals, p(parsed), p(compact), p(structs), structs.numel() if structs is not None else 0,
                  p(initial_sps_slot), p(initial_pps)]
        if want is None:
            self.lib.hbs_parse_headers_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                           C.c_void_p, C.c_void_p, C.c_void_p]
            self._check(self.lib.hbs_parse_headers_compact(*common, p(summary)), "hbs_parse_headers_compact")
        else:
            self.lib.hbs_parse_materialize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
            self._check(self.lib.hbs_parse_materialize(*common, p(want), want.numel(), p(summary)), "hbs_parse_materialize")

    def parse_headers_compact(self, rbsp, index, n_nals, want=None, poison=None):
        """Plan, allocate, parse: (parsed ndarray[PARSED], compact ndarray[COMPACT], structs device tensor holding the parameter
        sets and -- want: a list of NAL numbers -- the full slice headers of those NALs)."""
        t = self.torch
        dev = t.device("cuda", self.device)
        parsed = t.empty(max(n_nals, 1) * PARSED.itemsize, dtype=t.uint8, device=dev)
        compact = t.empty(max(n_nals, 1) * COMPACT.itemsize, dtype=t.uint8, device=dev)
        summary = t.zeros(SUMMARY.itemsize, dtype=t.uint8, device=dev)
        want_dev = None if want is None else t.as_tensor(np.asarray(want, dtype=np.int64), device=dev)
        self.parse_compact_async(rbsp, index, n_nals, parsed, compact, None, summary, want_dev)
        need = int(self.read_summary(summary)["reserved"][0])
        structs = t.empty(need + 16, dtype=t.uint8, device=dev)
        if poison is not None:
            structs.fill_(poison)
        self.parse_compact_async(rbsp, index, n_nals, parsed, compact, structs, summary, want_dev)
        s = self.read_summary(summary)
        if int(s["error"]) != 0:
            e = HbsError("hbs_parse_headers_compact: error %d" % int(s["error"]))
            e.code = int(s["error"])
            raise e
        return (parsed[: n_nals * PARSED.itemsize].cpu().numpy().view(PARSED).copy(),
                compact[: n_nals * COMPACT.itemsize].cpu().numpy().view(COMPACT).copy(), structs)

    def index_parse_compact_async(self, stream, index, index_cap, parsed, compact, structs, scan_summary, parse_summary, window=0, payload_off=None):
        """hbs_index_parse_compact: as index_parse_async with the compact parse behind the scan"""
        self._bind_stream()
        self.lib.hbs_index_parse_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        n = C.c_uint64(0)
        rc = self.lib.hbs_index_parse_compact(self.h, C.c_void_p(stream.data_ptr() if stream.numel() else None), stream.numel(),
                                              C.c_void_p(index.data_ptr()), index_cap, window, C.c_void_p(parsed.data_ptr()), C.c_void_p(compact.data_ptr()),
                                              C.c_void_p(structs.data_ptr()) if structs is not None else None,
                                              structs.numel() if structs is not None else 0,
                                              C.c_void_p(payload_off.data_ptr()) if payload_off is not None else None,
                                              C.c_void_p(scan_summary.data_ptr()), C.c_void_p(parse_summary.data_ptr()), C.byref(n))
        self._check(rc, "hbs_index_parse_compact")
        return int(n.value)

    def parse_extended(self, rbsp, index, n_nals, parsed_dev):
        """The NAL types the reference never dispatches (AUD, EOS, EOB, filler data, SEI), behind parse_headers on the same
        arrays: updates parsed_dev[k].rc for those NALs in place and returns the hbs_ext_nal records (ndarray[EXT_NAL])."""
        t = self.torch
        ext = t.empty(max(n_nals, 1) * EXT_NAL.itemsize, dtype=t.uint8, device=t.device("cuda", self.device))
        self._bind_stream()
        self.lib.hbs_parse_extended.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        self._check(self.lib.hbs_parse_extended(self.h, C.c_void_p(rbsp.data_ptr()), C.c_void_p(index.data_ptr()), n_nals,
                                                C.c_void_p(parsed_dev.data_ptr()), C.c_void_p(ext.data_ptr())), "hbs_parse_extended")
        return ext[: n_nals * EXT_NAL.itemsize].cpu().numpy().view(EXT_NAL).copy()

    def parse_headers(self, rbsp, index, n_nals, poison=None):
        """Plan, allocate the struct arena, parse.  Returns (parsed ndarray[PARSED], structs device tensor).
        poison: byte the arena is filled with beforehand (tests: the parse has to clear what it fills)."""
        t = self.torch
        dev = t.device("cuda", self.device)
        parsed = t.empty(max(n_nals, 1) * PARSED.itemsize, dtype=t.uint8, device=dev)
        summary = t.zeros(SUMMARY.itemsize, dtype=t.uint8, device=dev)
        self.parse_headers_async(rbsp, index, n_nals, parsed, None, summary)
        need = int(self.read_summary(summary)["reserved"][0])
        structs = t.empty(need + 16, dtype=t.uint8, device=dev)
        if poison is not None:
            structs.fill_(poison)
        self.parse_headers_async(rbsp, index, n_nals, parsed, structs, summary)
        s = self.read_summary(summary)
        if int(s["error"]) != 0:
            raise HbsError("hbs_parse_headers: error %d" % int(s["error"]))
        return parsed[: n_nals * PARSED.itemsize].cpu().numpy().view(PARSED).copy(), structs

    # ---- NAL filter -------------------------------------------------------------------

    @staticmethod
    def nal_filter(keep_types=NALMASK_ALL, max_temporal_id_plus1=7, max_layer_id=63, keep_short=True):
        """an hbs_nal_filter record (ndarray[NAL_FILTER] of one)"""
        r = np.zeros(1, dtype=NAL_FILTER)
        r["keep_types"] = int(keep_types) & NALMASK_ALL
        r["max_temporal_id_plus1"] = int(max_temporal_id_plus1)
        r["max_layer_id"] = int(max_layer_id)
        r["keep_short"] = 1 if keep_short else 0
        return r

    def filter_annexb_async(self, stream, stream_bytes, index, n_nals, out, index_out, summary, rule=None, keep=None, out_cap=None):
        """Enqueue hbs_filter_annexb on the current torch stream.  stream / index / out / index_out / summary / keep are device
        tensors (out None: plan only; index_out may be None); rule is an ndarray[NAL_FILTER] of one (host memory).  Exactly one of
        rule and keep is given.  Raises HbsError for arguments the call refuses (the later _async wrappers return the code)."""
        self._bind_stream()
        rule, rule_p = _rec(rule, NAL_FILTER)
        if out_cap is None:
            out_cap = _holds(out)
        rc = self.lib.hbs_filter_annexb(self.h, _p(stream) if stream_bytes else None, int(stream_bytes), _p(index) if n_nals else None,
                                        int(n_nals), rule_p, _p(keep), _p(out), int(out_cap), _p(index_out), _p(summary))
        self._check(rc, "hbs_filter_annexb")

    def filter_annexb(self, stream, index_entries, keep_types=NALMASK_ALL, max_temporal_id_plus1=7, max_layer_id=63,
                      keep_short=True, keep=None, stream_bytes=None):
        """Convenience: cut `stream` (device uint8 tensor) down to the NAL units a rule keeps -- or, keep given, those whose
        byte in `keep` (array of n_nals, non-zero = keep; host or device) is set.  index_entries: ndarray[NAL_ENTRY] (host) or a
        device uint8 tensor of its entries.  Plans first, allocates the exact output, runs.  Returns (out device tensor,
        entries_out ndarray[NAL_ENTRY], summary record)."""
        d_idx, n = self._dv(index_entries, NAL_ENTRY, empty=False)
        nbytes = int(stream.numel()) if stream_bytes is None else int(stream_bytes)
        rule = self.nal_filter(keep_types, max_temporal_id_plus1, max_layer_id, keep_short) if keep is None else None
        d_keep, _ = self._dv(keep, np.uint8)
        summary = self._zeros()
        self.filter_annexb_async(stream, nbytes, d_idx, n, None, None, summary, rule=rule, keep=d_keep)
        need = int(self._run("hbs_filter_annexb", 0, summary)["stream_bytes"])
        out = self._empty(max(need, 16))
        d_out_idx = self._empty(max(n, 1) * NAL_ENTRY.itemsize)
        self.filter_annexb_async(stream, nbytes, d_idx, n, out, d_out_idx, summary, rule=rule, keep=d_keep, out_cap=need)
        s = self._run("hbs_filter_annexb", 0, summary)
        return out[:need], _host(d_out_idx, int(s["nal_count"]), NAL_ENTRY), s

    # ---- length-prefixed NAL units (MP4 samples) ---------------------------------------

    def annexb_to_lenpref_async(self, stream, stream_bytes, index, n_nals, out, index_out, summary, keep=None, length_size=4,
                                nal_au=None, n_aus=0, sample_off=None, out_cap=None):
        """Enqueue hbs_annexb_to_lenpref on the current torch stream.  stream / index / out / index_out / summary / keep / nal_au /
        sample_off are device tensors (out None: plan only; index_out, keep, nal_au, sample_off may be None).  Returns the
        call's return code (0, or HBS_E_ARG for arguments it refuses)."""
        self._bind_stream()
        if out_cap is None:
            out_cap = _holds(out)
        return self.lib.hbs_annexb_to_lenpref(self.h, _p(stream) if stream_bytes else None, int(stream_bytes),
                                              _p(index) if n_nals else None, int(n_nals), _p(keep), int(length_size),
                                              _p(nal_au), int(n_aus), _p(sample_off), _p(out), int(out_cap), _p(index_out), _p(summary))

    def lenpref_to_annexb_async(self, data, in_bytes, sample_off, sample_size, n_samples, out, sample_off_out, summary,
                                length_size=4, startcode_bytes=4, nal_cap=0, out_cap=None):
        """Enqueue hbs_lenpref_to_annexb on the current torch stream.  data / sample_off / sample_size / out / sample_off_out /
        summary are device tensors (out None: plan only; sample_off_out may be None).  Returns the call's return code."""
        self._bind_stream()
        if out_cap is None:
            out_cap = _holds(out)
        return self.lib.hbs_lenpref_to_annexb(self.h, _p(data) if in_bytes else None, int(in_bytes), int(length_size),
                                              _p(sample_off) if n_samples else None, _p(sample_size) if n_samples else None,
                                              int(n_samples), int(startcode_bytes), int(nal_cap), _p(out), int(out_cap),
                                              _p(sample_off_out), _p(summary))

    def annexb_to_lenpref(self, stream, index_entries, keep=None, length_size=4, nal_au=None, n_aus=0, stream_bytes=None):
        """Convenience: the kept NAL units of `stream` (device uint8 tensor) as length-prefixed records.  index_entries:
        ndarray[NAL_ENTRY] (host) or a device uint8 tensor of its entries; keep: None (all) or n_nals bytes, host or device;
        nal_au: None or the AU number of every NAL (uint32, host or device) with n_aus, for the sample table.  Plans first,
        allocates the exact output, runs.  Returns (out device tensor, entries_out ndarray[NAL_ENTRY], sample_off ndarray[uint64]
        of n_aus + 1 or None, summary record)."""
        name = "hbs_annexb_to_lenpref"
        d_idx, n = self._dv(index_entries, NAL_ENTRY, empty=False)
        nbytes = int(stream.numel()) if stream_bytes is None else int(stream_bytes)
        d_keep, _ = self._dv(keep, np.uint8)
        d_au, _ = self._dv(nal_au, np.uint32)
        summary = self._zeros()
        args = dict(keep=d_keep, length_size=length_size, nal_au=d_au, n_aus=n_aus)
        s = self._run(name, self.annexb_to_lenpref_async(stream, nbytes, d_idx, n, None, None, summary, **args), summary)
        need = int(s["stream_bytes"])
        out = self._empty(max(need, 16))
        d_out_idx = self._empty(max(n, 1) * NAL_ENTRY.itemsize)
        d_so = self._empty((int(n_aus) + 1) * 8) if d_au is not None else None
        s = self._run(name, self.annexb_to_lenpref_async(stream, nbytes, d_idx, n, out, d_out_idx, summary, sample_off=d_so, out_cap=need, **args),
                      summary)
        return (out[:need], _host(d_out_idx, int(s["nal_count"]), NAL_ENTRY),
                d_so.cpu().numpy().view(np.uint64).copy() if d_so is not None else None, s)

    def _offsets_and_sizes(self, name, off, size, what):
        """two uint64 tables of one length, host or device -> (offsets on the device, sizes on the device, entries)"""
        d_off, n = self._dv(off, np.uint64)
        d_size, n2 = self._dv(size, np.uint64)
        if n != n2:
            raise HbsError("%s: %d %s offsets, %d sizes" % (name, n, what, n2))
        return d_off, d_size, n

    def lenpref_to_annexb(self, data, sample_off, sample_size, length_size=4, startcode_bytes=4, in_bytes=None):
        """Convenience: the samples data[off_s, off_s + size_s) (sample_off / sample_size: uint64 arrays, host or device
        tensors of their bytes) as one Annex-B stream.  Plans first, allocates the exact output, runs.  Returns (out device
        tensor, sample_off_out ndarray[uint64] of n_samples + 1, summary record)."""
        name = "hbs_lenpref_to_annexb"
        d_off, d_size, n = self._offsets_and_sizes(name, sample_off, sample_size, "sample")
        nbytes = int(data.numel()) if in_bytes is None else int(in_bytes)
        summary = self._zeros()
        args = dict(length_size=length_size, startcode_bytes=startcode_bytes)
        s = self._run(name, self.lenpref_to_annexb_async(data, nbytes, d_off, d_size, n, None, None, summary, nal_cap=(1 << 64) - 1, **args),
                      summary, " (sample {0})")
        need, recs = int(s["stream_bytes"]), int(s["nal_count"])
        out = self._empty(max(need, 16))
        d_so = self._empty((n + 1) * 8)
        s = self._run(name, self.lenpref_to_annexb_async(data, nbytes, d_off, d_size, n, out, d_so, summary, nal_cap=recs, out_cap=need, **args),
                      summary)
        return out[:need], d_so.cpu().numpy().view(np.uint64).copy(), s

    # ---- MPEG transport stream -----------------------------------------------------------

    def ts_demux_async(self, ts, ts_bytes, packet_bytes, pid, out, pes, summary, out_cap=None, pes_cap=None):
        """Enqueue hbs_ts_demux on the current torch stream.  ts / out / pes / summary are device tensors (out None: plan only;
        pes may be None).  Returns the call's return code (0, or HBS_E_ARG for arguments it refuses)."""
        self._bind_stream()
        if out_cap is None:
            out_cap = _holds(out)
        if pes_cap is None:
            pes_cap = _holds(pes, TS_PES.itemsize)
        return self.lib.hbs_ts_demux(self.h, _p(ts) if ts_bytes else None, int(ts_bytes), int(packet_bytes), int(pid),
                                     _p(out), int(out_cap), _p(pes), int(pes_cap), _p(summary))

    def ts_demux(self, ts, pid, packet_bytes=188, ts_bytes=None):
        """Convenience: the elementary stream of `pid` in the transport stream `ts` (device uint8 tensor).  Plans first,
        allocates the exact outputs, runs.  Returns (out device tensor, pes ndarray[TS_PES], summary record)."""
        name = "hbs_ts_demux"
        nbytes = int(ts.numel()) if ts_bytes is None else int(ts_bytes)
        summary = self._zeros()
        s = self._run(name, self.ts_demux_async(ts, nbytes, packet_bytes, pid, None, None, summary), summary, " (packet {0})")
        need, n_pes = int(s["stream_bytes"]), int(s["nal_count"])
        out = self._empty(max(need, 16))
        pes = self._empty(max(n_pes, 1) * TS_PES.itemsize)
        s = self._run(name, self.ts_demux_async(ts, nbytes, packet_bytes, pid, out, pes, summary, out_cap=need, pes_cap=n_pes), summary)
        return out[:need], _host(pes, n_pes, TS_PES), s

    def ts_mux_async(self, stream, stream_bytes, au, n_aus, pts, dts, params, out, au_packet, summary, out_cap=None):
        """Enqueue hbs_ts_mux on the current torch stream.  stream / au / pts / dts / out / au_packet / summary are device
        tensors (pts, dts, au_packet may be None; out None: plan only); params is an ndarray[TS_MUX_PARAMS] of one in host
        memory.  Returns the call's return code (0, or HBS_E_ARG for arguments it refuses)."""
        self._bind_stream()
        if out_cap is None:
            out_cap = _holds(out)
        params, params_p = _rec(params, TS_MUX_PARAMS)
        return self.lib.hbs_ts_mux(self.h, _p(stream) if stream_bytes else None, int(stream_bytes), _p(au) if n_aus else None, int(n_aus),
                                   _p(pts), _p(dts), params_p, _p(out), int(out_cap), _p(au_packet), _p(summary))

    def ts_mux(self, stream, au, pts=None, dts=None, stream_bytes=None, **params):
        """Convenience: the access units `au` (ndarray[ACCESS_UNIT] or a device uint8 tensor of the records) of `stream` (device
        uint8 tensor) as transport packets.  pts / dts: None or one uint64 per AU (TS_NO_TIME: absent), host arrays or device
        tensors; params: the keywords of ts_mux_params.  Plans first, allocates the exact output, runs.  Returns (out device
        tensor, au_packet ndarray[uint32] of n_aus + 1, summary record)."""
        name = "hbs_ts_mux"
        au, n = self._dv(au, ACCESS_UNIT)
        pts, dts = self._dv(pts, np.uint64)[0], self._dv(dts, np.uint64)[0]
        prm = ts_mux_params(**params)
        nbytes = int(stream.numel()) if stream_bytes is None else int(stream_bytes)
        summary = self._zeros()
        s = self._run(name, self.ts_mux_async(stream, nbytes, au, n, pts, dts, prm, None, None, summary), summary, " (access unit {0})")
        need = int(s["stream_bytes"])
        out = self._empty(max(need, 16))
        au_packet = self.torch.empty(n + 1, dtype=self.torch.int32, device=out.device)
        s = self._run(name, self.ts_mux_async(stream, nbytes, au, n, pts, dts, prm, out, au_packet, summary, out_cap=need), summary)
        return out[:need], au_packet.cpu().numpy().view(np.uint32).copy(), s

    # ---- RTP ------------------------------------------------------------------------------

    def rtp_pack_async(self, stream, stream_bytes, index, n_nals, nal_au, n_aus, pts, params, out, nal_off, nal_packet, summary, out_cap=None):
        """Enqueue hbs_rtp_pack on the current torch stream.  stream / index / nal_au / pts / out / nal_off / nal_packet / summary
        are device tensors (nal_au, pts, nal_off, nal_packet may be None; out None: plan only); params is an
        ndarray[RTP_PARAMS] of one in host memory.  Returns the call's return code (0, or HBS_E_ARG for arguments it refuses)."""
        self._bind_stream()
        if out_cap is None:
            out_cap = _holds(out)
        params, params_p = _rec(params, RTP_PARAMS)
        return self.lib.hbs_rtp_pack(self.h, _p(stream) if stream_bytes else None, int(stream_bytes), _p(index) if n_nals else None, int(n_nals),
                                     _p(nal_au), int(n_aus), _p(pts), params_p, _p(out), int(out_cap), _p(nal_off), _p(nal_packet), _p(summary))

    def rtp_pack(self, stream, index, n_nals=None, nal_au=None, n_aus=None, pts=None, stream_bytes=None, **params):
        """Convenience: the NALs `index` (ndarray[NAL_ENTRY] or a device uint8 tensor of the records) of `stream` (device uint8
        tensor) as RTP packets.  nal_au: None or one uint32 per NAL; pts: None or one uint64 per AU; host arrays or device
        tensors; params: the keywords of rtp_params.  Plans first, allocates the exact output, runs.  Returns (out device
        tensor, packet_off ndarray[uint64] of packets + 1: where every packet begins and the total, summary record)."""
        name = "hbs_rtp_pack"
        index, n = self._dv(index, NAL_ENTRY)
        if n_nals is not None:
            n = n_nals
        nal_au, pts_given = self._dv(nal_au, np.uint32)[0], pts is not None
        pts, n_pts = self._dv(pts, np.uint64)
        if n_aus is None:                                   # the times say how many AUs there are; AU numbers without times: any
            n_aus = n_pts if pts_given or nal_au is None else 1 << 32
        prm = rtp_params(**params)
        nbytes = int(stream.numel()) if stream_bytes is None else int(stream_bytes)
        summary = self._zeros()
        args = (stream, nbytes, index, n, nal_au, n_aus, pts, prm)
        s = self._run(name, self.rtp_pack_async(*args, None, None, None, summary), summary, " (NAL {0})")
        need = int(s["stream_bytes"])
        out = self._empty(max(need, 16))
        nal_off, nal_packet = (self._empty((n + 1) * 8) for _ in range(2))
        s = self._run(name, self.rtp_pack_async(*args, out, nal_off, nal_packet, summary, out_cap=need), summary)
        tabs = [x.cpu().numpy().view(np.uint64) for x in (nal_off, nal_packet)]
        return out[:need], rtp_packet_offsets(tabs[0], tabs[1], int(prm["max_payload"][0]), int(prm["framing"][0])), s

    def rtp_unpack_async(self, data, in_bytes, pkt_off, pkt_size, n_packets, params, out, index_out, nal_au_out, au_ts_out, summary,
                         out_cap=None, nal_cap=None, au_cap=None):
        """Enqueue hbs_rtp_unpack on the current torch stream.  data / pkt_off / pkt_size / out / index_out / nal_au_out /
        au_ts_out / summary are device tensors (index_out, nal_au_out, au_ts_out may be None; out None: plan only); params is
        an ndarray[RTP_UNPACK_PARAMS] of one in host memory.  nal_cap / au_cap default to what the tensors hold.  Returns the
        call's return code (0, or HBS_E_ARG for arguments it refuses)."""
        self._bind_stream()
        if out_cap is None:
            out_cap = _holds(out)
        if nal_cap is None:
            caps = [_holds(x, w) for x, w in ((index_out, NAL_ENTRY.itemsize), (nal_au_out, 4)) if x is not None]
            nal_cap = min(caps) if caps else (1 << 64) - 1
        if au_cap is None:
            au_cap = _holds(au_ts_out, 8)
        params, params_p = _rec(params, RTP_UNPACK_PARAMS)
        return self.lib.hbs_rtp_unpack(self.h, _p(data) if in_bytes else None, int(in_bytes), _p(pkt_off) if n_packets else None,
                                       _p(pkt_size) if n_packets else None, int(n_packets), params_p, _p(out), int(out_cap),
                                       _p(index_out), _p(nal_au_out), int(nal_cap), _p(au_ts_out), int(au_cap), _p(summary))

    def rtp_unpack(self, data, pkt_off, pkt_size, in_bytes=None, **params):
        """Convenience: the RTP packets data[off_p, off_p + size_p) (data: device uint8 tensor; pkt_off / pkt_size: uint64 arrays,
        host or device tensors of their bytes) as one Annex-B stream; params: the keywords of rtp_unpack_params.  Plans first,
        allocates the exact outputs, runs.  Returns (out device tensor, index device tensor of NAL_ENTRY records, nal_au
        ndarray[uint32], au_ts ndarray[uint64], summary record)."""
        name = "hbs_rtp_unpack"
        d_off, d_size, n = self._offsets_and_sizes(name, pkt_off, pkt_size, "packet")
        prm = rtp_unpack_params(**params)
        nbytes = int(data.numel()) if in_bytes is None else int(in_bytes)
        summary = self._zeros()
        args = (data, nbytes, d_off, d_size, n, prm)
        s = self._run(name, self.rtp_unpack_async(*args, None, None, None, None, summary), summary, " (packet {0})")
        need, nals, aus = int(s["stream_bytes"]), int(s["nal_count"]), int(s["reserved"][1])
        out = self._empty(max(need, 16))
        index = self._empty(max(nals, 1) * NAL_ENTRY.itemsize)
        nal_au = self._empty(max(nals, 1) * 4)
        au_ts = self._empty(max(aus, 1) * 8)
        s = self._run(name, self.rtp_unpack_async(*args, out, index, nal_au, au_ts, summary, out_cap=need, nal_cap=nals, au_cap=aus), summary)
        return out[:need], index[: nals * NAL_ENTRY.itemsize], _host(nal_au, nals, np.uint32), _host(au_ts, aus, np.uint64), s

    def rtp_order_async(self, data, in_bytes, pkt_off, pkt_size, n_packets, params, off_out, size_out, src_out, ext_out, summary,
                        out_cap=None):
        """Enqueue hbs_rtp_order on the current torch stream.  data / pkt_off / pkt_size / off_out / size_out / src_out / ext_out /
        summary are device tensors (src_out, ext_out may be None; off_out and size_out None: plan only); params is an
        ndarray[RTP_ORDER_PARAMS] of one in host memory.  out_cap (entries) defaults to what the tensors hold.  Returns the
        call's return code (0, or HBS_E_ARG for arguments it refuses)."""
        self._bind_stream()
        if out_cap is None:
            caps = [_holds(x, w) for x, w in ((off_out, 8), (size_out, 8), (src_out, 4), (ext_out, 8)) if x is not None]
            out_cap = min(caps) if caps else 0
        params, params_p = _rec(params, RTP_ORDER_PARAMS)
        return self.lib.hbs_rtp_order(self.h, _p(data) if in_bytes else None, int(in_bytes), _p(pkt_off) if n_packets else None,
                                      _p(pkt_size) if n_packets else None, int(n_packets), params_p, _p(off_out), _p(size_out),
                                      _p(src_out), _p(ext_out), int(out_cap), _p(summary))

    def rtp_order(self, data, pkt_off, pkt_size, in_bytes=None, **params):
        """Convenience: the table of the RTP packets data[off_p, off_p + size_p) in arrival order (data: device uint8 tensor;
        pkt_off / pkt_size: uint64 arrays, host or device tensors of their bytes) by sequence number, each packet once; params:
        the keywords of rtp_order_params (max_span defaults to n_packets + 65536).  Plans first, allocates the exact outputs,
        runs.  Returns (off device tensor, size device tensor -- the bytes of uint64 tables, what rtp_unpack takes --, src
        ndarray[uint32], ext ndarray[uint64], summary record)."""
        name = "hbs_rtp_order"
        d_off, d_size, n = self._offsets_and_sizes(name, pkt_off, pkt_size, "packet")
        params.setdefault("max_span", n + 65536)
        prm = rtp_order_params(**params)
        nbytes = int(data.numel()) if in_bytes is None else int(in_bytes)
        summary = self._zeros()
        args = (data, nbytes, d_off, d_size, n, prm)

        def where(s):                                       # a faulty packet is named; otherwise the span was too long
            return " (packet {0})" if int(s["reserved"][0]) else " (span %d, max_span %d)" % (int(s["stream_bytes"]), int(prm["max_span"][0]))
        s = self._run(name, self.rtp_order_async(*args, None, None, None, None, summary), summary, where)
        kept = int(s["nal_count"])
        off, size, ext = (self._empty(max(kept, 1) * 8) for _ in range(3))
        src = self._empty(max(kept, 1) * 4)
        s = self._run(name, self.rtp_order_async(*args, off, size, src, ext, summary, out_cap=kept), summary)
        return off[: kept * 8], size[: kept * 8], _host(src, kept, np.uint32), _host(ext, kept, np.uint64), s

    # ---- fragmented MP4 -----------------------------------------------------------------

    def mp4_fragment_async(self, stream, stream_bytes, index, n_nals, nal_au, au, n_aus, params, out, summary, keep=None, dts=None,
                           pts=None, sample_off=None, sample_size=None, frag=None, frag_cap=None, out_cap=None):
        """Enqueue hbs_mp4_fragment on the current torch stream.  stream / index / nal_au / au / out / summary / keep / dts / pts /
        sample_off / sample_size / frag are device tensors (out None: plan only; keep, dts, pts, sample_off with sample_size and
        frag may be None); params is an ndarray[MP4_PARAMS] of one in host memory.  frag_cap (records) and out_cap (bytes)
        default to what the tensors hold.  Returns the call's return code (0, or HBS_E_ARG for arguments it refuses)."""
        self._bind_stream()
        if out_cap is None:
            out_cap = _holds(out)
        if frag_cap is None:
            frag_cap = _holds(frag, MP4_FRAG.itemsize)
        params, params_p = _rec(params, MP4_PARAMS)
        return self.lib.hbs_mp4_fragment(self.h, _p(stream) if stream_bytes else None, int(stream_bytes), _p(index) if n_nals else None,
                                         int(n_nals), _p(keep), _p(nal_au) if n_nals else None, _p(au) if n_aus else None, int(n_aus),
                                         _p(dts), _p(pts), params_p, _p(out), int(out_cap), _p(sample_off), _p(sample_size), _p(frag),
                                         int(frag_cap), _p(summary))

    def mp4_fragment(self, stream, index, nal_au, au, keep=None, dts=None, pts=None, stream_bytes=None, **params):
        """Convenience: the access units of `stream` (device uint8 tensor) as fMP4 fragments.  index: ndarray[NAL_ENTRY], nal_au:
        one uint32 per NAL, au: ndarray[ACCESS_UNIT], keep: None or a byte per NAL, dts / pts: None or one uint64 per AU -- host
        arrays or device uint8 tensors of their bytes; params: the keywords of mp4_params.  Plans first, allocates the exact
        output, runs.  Returns (out device tensor, sample_off ndarray[uint64], sample_size ndarray[uint64],
        frags ndarray[MP4_FRAG], summary record)."""
        name = "hbs_mp4_fragment"
        index, n = self._dv(index, NAL_ENTRY)
        au, n_aus = self._dv(au, ACCESS_UNIT)
        nal_au, keep = self._dv(nal_au, np.uint32)[0], self._dv(keep, np.uint8)[0]
        dts, pts = self._dv(dts, np.uint64)[0], self._dv(pts, np.uint64)[0]
        prm = mp4_params(**params)
        nbytes = int(stream.numel()) if stream_bytes is None else int(stream_bytes)
        summary = self._zeros()
        args = (stream, nbytes, index, n, nal_au, au, n_aus, prm)
        kw = dict(keep=keep, dts=dts, pts=pts)
        s = self._run(name, self.mp4_fragment_async(*args, None, summary, **kw), summary, " (NAL {0}, access unit {1})")
        need, frags = int(s["stream_bytes"]), int(s["nal_count"])
        out = self._empty(max(need, 16))
        so, ss = (self._empty(max(n_aus, 1) * 8) for _ in range(2))
        fr = self._empty(max(frags, 1) * MP4_FRAG.itemsize)
        s = self._run(name, self.mp4_fragment_async(*args, out, summary, sample_off=so, sample_size=ss, frag=fr, frag_cap=frags, out_cap=need, **kw),
                      summary)
        return out[:need], _host(so, n_aus, np.uint64), _host(ss, n_aus, np.uint64), _host(fr, frags, MP4_FRAG), s

    def mp4_samples_async(self, data, in_bytes, params, summary, seg=None, seg_stride=16, n_segs=0, moof_cap=0, sample_cap=0,
                          sample_off=None, sample_size=None, dts=None, pts=None, sample_flags=None, frag=None):
        """Enqueue hbs_mp4_samples on the current torch stream.  data / summary / seg / sample_off / sample_size / dts / pts /
        sample_flags / frag are device tensors (seg None: one segment, the buffer; sample_off with sample_size None: plan only;
        dts, pts, sample_flags, frag may be None); params is an ndarray[MP4_READ_PARAMS] of one in host memory.  Returns the
        call's return code (0, or HBS_E_ARG for arguments it refuses)."""
        self._bind_stream()
        params, params_p = _rec(params, MP4_READ_PARAMS)
        return self.lib.hbs_mp4_samples(self.h, _p(data) if in_bytes else None, int(in_bytes), _p(seg), int(seg_stride), int(n_segs),
                                        params_p, int(moof_cap), int(sample_cap), _p(sample_off), _p(sample_size), _p(dts), _p(pts),
                                        _p(sample_flags), _p(frag), _p(summary))

    def mp4_samples(self, data, seg=None, seg_stride=None, in_bytes=None, moof_cap=None, **params):
        """Convenience: the sample table of the fMP4 segments in `data` (device uint8 tensor).  seg: None (one segment, the
        buffer), an (n, 2) uint64 host array of offsets and sizes, an ndarray[MP4_FRAG], or a device uint8 tensor of records with
        seg_stride (default 16); moof_cap: the most moofs the plan has room for (default: in_bytes // 8, at most 4096; the plan
        is run again with the count when that was too few); params: the keywords of mp4_read_params.  Plans, allocates the
        exact tables, runs.  Returns (sample_off, sample_size, dts, pts, flags, frags ndarray[MP4_FRAG], summary record), host
        arrays."""
        name = "hbs_mp4_samples"
        nbytes = int(data.numel()) if in_bytes is None else int(in_bytes)
        n_segs = 0
        if isinstance(seg, np.ndarray):
            if seg.dtype == MP4_FRAG:
                seg_stride = MP4_FRAG.itemsize
            else:
                seg, seg_stride = np.ascontiguousarray(seg, dtype=np.uint64).reshape(-1, 2), 16
            seg, n_segs = self._dv(seg)
        elif seg is not None:
            seg_stride = 16 if seg_stride is None else int(seg_stride)
            n_segs = _holds(seg, seg_stride)
        prm = mp4_read_params(**params)
        summary = self._zeros()
        kw = dict(seg=seg, seg_stride=seg_stride or 16, n_segs=n_segs)
        cap = min(nbytes // 8, 4096) if moof_cap is None else int(moof_cap)
        for _ in range(2):
            self._check(self.mp4_samples_async(data, nbytes, prm, summary, moof_cap=cap, **kw), name)
            s = self.read_summary(summary)
            if int(s["error"]) == -4 and int(s["nal_found"]) > cap:          # HBS_E_CAPACITY: the default was too small
                cap = int(s["nal_found"])
                continue
            break
        self._raise_on(name, s, " (segment {0}, moof {1}, sample {2})")
        n, m = int(s["nal_count"]), int(s["nal_found"])
        so, ss, dt, pt = (self._empty(max(n, 1) * 8) for _ in range(4))
        fl = self._empty(max(n, 1) * 4)
        fr = self._empty(max(m, 1) * MP4_FRAG.itemsize)
        s = self._run(name, self.mp4_samples_async(data, nbytes, prm, summary, moof_cap=m, sample_cap=n, sample_off=so, sample_size=ss, dts=dt,
                                                   pts=pt, sample_flags=fl, frag=fr, **kw), summary)
        return (*(_host(x, n, np.uint64) for x in (so, ss, dt, pt)), _host(fl, n, np.uint32), _host(fr, m, MP4_FRAG), s)

    def mp4_protect_async(self, data, in_bytes, frag, n_frags, sub_first, sub, iv, n_samples, params, out, summary, sample_off=None,
                          sample_size=None, frag_out=None, out_cap=None):
        """Enqueue hbs_mp4_protect on the current torch stream.  data / frag / sub_first / sub / iv / out / summary / sample_off /
        sample_size / frag_out are device tensors (out None: plan only; iv may be None with iv_size 0; sample_off with
        sample_size and frag_out may be None); params is an ndarray[MP4_PROTECT_PARAMS] of one in host memory.  out_cap (bytes)
        defaults to what out holds.  Returns the call's return code (0, or HBS_E_ARG for arguments it refuses)."""
        self._bind_stream()
        if out_cap is None:
            out_cap = _holds(out)
        params, params_p = _rec(params, MP4_PROTECT_PARAMS)
        on = bool(n_samples)
        return self.lib.hbs_mp4_protect(self.h, _p(data) if in_bytes else None, int(in_bytes), _p(frag) if n_frags else None, int(n_frags),
                                        _p(sub_first) if on else None, _p(sub) if on else None, _p(iv), int(n_samples), params_p, _p(out),
                                        int(out_cap), _p(sample_off), _p(sample_size), _p(frag_out), _p(summary))

    def mp4_protect(self, data, frags, sub_first, sub, iv=None, iv_size=8, in_bytes=None):
        """Convenience: the fragments of `data` (device uint8 tensor) that `frags` names, with saiz, saio and senc in every traf.
        frags: ndarray[MP4_FRAG]; sub_first: one uint64 per sample and one; sub: ndarray[CENC_SUBSAMPLE]; iv: None (iv_size 0) or
        16 bytes per sample -- host arrays or device uint8 tensors of their bytes.  Plans first, allocates the exact output,
        runs.  Returns (out device tensor, sample_off ndarray[uint64], sample_size ndarray[uint64], frags ndarray[MP4_FRAG],
        summary record)."""
        name = "hbs_mp4_protect"
        d_frag, n_frags = self._dv(frags, MP4_FRAG)
        d_first, n1 = self._dv(sub_first, np.uint64)
        d_sub, _ = self._dv(sub, CENC_SUBSAMPLE)
        d_iv, _ = self._dv(iv, np.uint8)
        n = max(n1 - 1, 0)
        prm = mp4_protect_params(iv_size=iv_size)
        nbytes = int(data.numel()) if in_bytes is None else int(in_bytes)
        summary = self._zeros()
        args = (data, nbytes, d_frag, n_frags, d_first, d_sub, d_iv, n, prm)
        s = self._run(name, self.mp4_protect_async(*args, None, summary), summary, " (sample {0}, fragment {1})")
        need = int(s["stream_bytes"])
        out = self._empty(max(need, 16))
        so, ss = (self._empty(max(n, 1) * 8) for _ in range(2))
        fr = self._empty(max(n_frags, 1) * MP4_FRAG.itemsize)
        s = self._run(name, self.mp4_protect_async(*args, out, summary, sample_off=so, sample_size=ss, frag_out=fr, out_cap=need), summary)
        return out[:need], _host(so, n, np.uint64), _host(ss, n, np.uint64), _host(fr, n_frags, MP4_FRAG), s

    def mp4_senc_samples_async(self, data, in_bytes, frag, n_frags, sample_size, n_samples, params, sub_first, sub, iv, summary, sub_cap=None):
        """Enqueue hbs_mp4_senc_samples on the current torch stream.  data / frag / sample_size / sub_first / sub / iv / summary are
        device tensors (sample_size may be None; sub None: plan only; iv may be None with iv_size 0); params is an
        ndarray[MP4_SENC_PARAMS] of one in host memory.  sub_cap (entries) defaults to what sub holds.  Returns the call's
        return code (0, or HBS_E_ARG for arguments it refuses)."""
        self._bind_stream()
        if sub_cap is None:
            sub_cap = _holds(sub, CENC_SUBSAMPLE.itemsize)
        params, params_p = _rec(params, MP4_SENC_PARAMS)
        return self.lib.hbs_mp4_senc_samples(self.h, _p(data) if in_bytes else None, int(in_bytes), _p(frag) if n_frags else None, int(n_frags),
                                             _p(sample_size), int(n_samples), params_p, _p(sub_first), _p(sub), int(sub_cap), _p(iv),
                                             _p(summary))

    def mp4_senc_samples(self, data, frags, sample_size=None, iv_size=8, track_id=0, flags=0, in_bytes=None, n_samples=None):
        """Convenience: the subsample table and the IVs of the protected fragments of `data` (device uint8 tensor) that `frags`
        (ndarray[MP4_FRAG], as mp4_samples returns it) names.  sample_size: None or one uint64 per sample, a host array or a
        device uint8 tensor of its bytes; n_samples: default the sum of the fragments' samples.  Plans first, allocates the exact
        tables, runs.  Returns (sub_first device tensor, sub device tensor, iv device tensor or None, summary record): device
        uint8 tensors of the tables' bytes, in the form cenc_crypt and cbcs_crypt take."""
        name = "hbs_mp4_senc_samples"
        d_frag, n_frags = self._dv(frags, MP4_FRAG)
        d_size, _ = self._dv(sample_size, np.uint64)
        n = int(np.asarray(frags)["samples"].sum()) if n_samples is None else int(n_samples)
        prm = mp4_senc_params(iv_size=iv_size, track_id=track_id, flags=flags)
        nbytes = int(data.numel()) if in_bytes is None else int(in_bytes)
        summary = self._zeros()
        first = self._empty((n + 1) * 8)
        iv = self._empty(max(n, 1) * 16) if iv_size else None
        args = (data, nbytes, d_frag, n_frags, d_size, n, prm, first)
        s = self._run(name, self.mp4_senc_samples_async(*args, None, iv, summary), summary, " (sample {0}, fragment {1})")
        total = int(s["nal_count"])
        sub = self._empty(max(total, 1) * CENC_SUBSAMPLE.itemsize)
        s = self._run(name, self.mp4_senc_samples_async(*args, sub, iv, summary, sub_cap=total), summary)
        return first, sub[: total * CENC_SUBSAMPLE.itemsize], (iv[: n * 16] if iv is not None else None), s

    def mp4_stbl_samples_async(self, data, in_bytes, tables, summary, sample_cap=0, sample_off=None, sample_size=None, dts=None, pts=None,
                               sample_flags=None):
        """Enqueue hbs_mp4_stbl_samples on the current torch stream.  data / summary / sample_off / sample_size / dts / pts /
        sample_flags are device tensors (sample_off with sample_size None: plan only; dts, pts, sample_flags may be None); tables
        is an ndarray[MP4_STBL] of one in host memory (mp4_stbl_find).  Returns the call's return code (0, or HBS_E_ARG for
        arguments it refuses)."""
        self._bind_stream()
        tables, tables_p = _rec(tables, MP4_STBL)
        return self.lib.hbs_mp4_stbl_samples(self.h, _p(data), int(in_bytes), tables_p, int(sample_cap), _p(sample_off), _p(sample_size),
                                             _p(dts), _p(pts), _p(sample_flags), _p(summary))

    def mp4_stbl_samples(self, data, tables, in_bytes=None):
        """Convenience: the sample table of the progressive MP4 whose table boxes lie in `data` (device uint8 tensor) where
        `tables` (mp4_stbl_find) says.  Plans, allocates the exact tables, runs.  Returns (sample_off, sample_size, dts, pts,
        flags, summary record), host arrays."""
        name = "hbs_mp4_stbl_samples"
        nbytes = int(data.numel()) if in_bytes is None else int(in_bytes)
        summary = self._zeros()
        s = self._run(name, self.mp4_stbl_samples_async(data, nbytes, tables, summary), summary, " (box {0})")
        n = int(s["nal_count"])
        if n > 0xFFFFFFFF:
            raise HbsError("hbs_mp4_stbl_samples: %d samples" % n)
        so, ss, dt, pt = (self._empty(max(n, 1) * 8) for _ in range(4))
        fl = self._empty(max(n, 1) * 4)
        s = self._run(name, self.mp4_stbl_samples_async(data, nbytes, tables, summary, sample_cap=n, sample_off=so, sample_size=ss, dts=dt, pts=pt,
                                                        sample_flags=fl), summary, " (sample {2})")
        return (*(_host(x, n, np.uint64) for x in (so, ss, dt, pt)), _host(fl, n, np.uint32), s)

    def mp4_stbl_write_async(self, sample_off, sample_size, n_samples, params, summary, dts=None, pts=None, sample_flags=None, out=None,
                             out_cap=0, tables=None):
        """Enqueue hbs_mp4_stbl_write on the current torch stream.  sample_off / sample_size / dts / pts / sample_flags / out /
        tables / summary are device tensors (dts, pts, sample_flags, tables may be None; out None: plan only); params is an
        ndarray[MP4_STBL_WRITE_PARAMS] of one in host memory (mp4_stbl_write_params).  Returns the call's return code (0, or
        HBS_E_ARG for arguments it refuses)."""
        self._bind_stream()
        params, params_p = _rec(params, MP4_STBL_WRITE_PARAMS)
        return self.lib.hbs_mp4_stbl_write(self.h, _p(sample_off), _p(sample_size), int(n_samples), _p(dts), _p(pts), _p(sample_flags),
                                           params_p, _p(out), int(out_cap), _p(tables), _p(summary))

    def mp4_stbl_write(self, sample_off, sample_size, n_samples, params, dts=None, pts=None, sample_flags=None):
        """Convenience: the sample table boxes of the samples in the device tables.  Plans, allocates the exact output, runs.
        Returns (boxes: device uint8 tensor of exactly T bytes, tables: ndarray[MP4_STBL] of one, summary record)."""
        name = "hbs_mp4_stbl_write"
        summary = self._zeros()
        rec = self._zeros(MP4_STBL.itemsize)
        kw = dict(dts=dts, pts=pts, sample_flags=sample_flags)
        s = self._run(name, self.mp4_stbl_write_async(sample_off, sample_size, n_samples, params, summary, **kw), summary, " (sample {2}, box {0})")
        total = int(s["stream_bytes"])
        out = self._empty(total)
        s = self._run(name, self.mp4_stbl_write_async(sample_off, sample_size, n_samples, params, summary, out=out, out_cap=total, tables=rec, **kw),
                      summary)
        return out, rec.cpu().numpy().view(MP4_STBL).copy(), s

    # ---- access units -----------------------------------------------------------------

    def access_units_async(self, index, parsed, compact, structs, n_nals, au, au_cap, nal_au, carry_out, summary, carry=None):
        """Enqueue hbs_access_units on the current torch stream.  index / parsed / compact / structs / au / nal_au / carry_out /
        summary are device tensors (structs, nal_au, carry_out may be None; au None: plan only); carry is an ndarray[AU_CARRY]
        of one (host memory) or None.  Returns the call's return code (0, or HBS_E_ARG for arguments it refuses)."""
        self._bind_stream()
        carry, carry_p = _rec(carry, AU_CARRY)
        return self.lib.hbs_access_units(self.h, _p(index), _p(parsed), _p(compact), _p(structs), int(n_nals), carry_p,
                                         _p(au), int(au_cap), _p(nal_au), _p(carry_out), _p(summary))

    def access_units(self, index, parsed, compact, structs, n_nals, carry=None):
        """Plan, allocate, run.  index / parsed / compact: device uint8 tensors of the records (or host ndarrays of them),
        structs: the struct arena (device tensor) or None.  Returns (au ndarray[ACCESS_UNIT], nal_au ndarray[uint32],
        summary record, carry_out ndarray[AU_CARRY] of one)."""
        name = "hbs_access_units"
        index, parsed, compact = (self._dv(x)[0] for x in (index, parsed, compact))
        summary = self._zeros()
        self._check(self.access_units_async(index, parsed, compact, structs, n_nals, None, 0, None, None, summary, carry), name)
        aus = int(self.read_summary(summary)["nal_count"])          # (the run reports what the plan found wrong as well)
        au = self._empty(max(aus, 1) * ACCESS_UNIT.itemsize)
        nal_au = self.torch.empty(max(n_nals, 1), dtype=self.torch.int32, device=au.device)
        carry_out = self._zeros(AU_CARRY.itemsize)
        s = self._run(name, self.access_units_async(index, parsed, compact, structs, n_nals, au, aus, nal_au, carry_out, summary, carry), summary)
        return _host(au, aus, ACCESS_UNIT), nal_au[:n_nals].cpu().numpy().view(np.uint32).copy(), s, carry_out.cpu().numpy().view(AU_CARRY).copy()

    def au_times_async(self, au, n_aus, params, summary, dts=None, pts=None, order=None, display=None):
        """Enqueue hbs_au_times on the current torch stream.  au / summary / dts / pts / order / display are device tensors (each
        of the four outputs may be None; all None: plan only), au may begin anywhere in an AU table (a GOP cut: a slice of the
        tensor); params is an ndarray[AU_TIMES_PARAMS] of one in host memory.  Returns the call's return code (0, or HBS_E_ARG
        for arguments it refuses)."""
        self._bind_stream()
        params, params_p = _rec(params, AU_TIMES_PARAMS)
        return self.lib.hbs_au_times(self.h, _p(au) if n_aus else None, int(n_aus), params_p, _p(dts), _p(pts), _p(order), _p(display),
                                     _p(summary))

    def au_times(self, au, tick=1, base_time=0, delay=None, flags=0):
        """Convenience: decode and presentation times of the access units `au` (ndarray[ACCESS_UNIT] or a device uint8 tensor of
        the records).  Returns (dts, pts, order, display, summary): device tensors (int64 views of the uint64 times, int32 of the
        uint32 slots) of one entry per AU, and the summary record."""
        t = self.torch
        au, n = self._dv(au, ACCESS_UNIT)
        prm = au_times_params(tick, base_time, delay, flags)
        summary = self._zeros()
        dts, pts = (t.empty(max(n, 1), dtype=t.int64, device=summary.device) for _ in range(2))
        order, display = (t.empty(max(n, 1), dtype=t.int32, device=summary.device) for _ in range(2))
        s = self._run("hbs_au_times", self.au_times_async(au, n, prm, summary, dts, pts, order, display), summary,
                      " (access unit {0} reorders across more than %d others)" % AUT_MAX_SPAN)
        return dts[:n], pts[:n], order[:n], display[:n], s

    # ---- Common Encryption: the subsample table, AES-128-CTR in place ------------------------------

    def cenc_subsamples_async(self, stream, stream_bytes, index, n_nals, nal_au, n_aus, params, sub_first, sub, summary, keep=None,
                              payload_off=None, sub_cap=None):
        """Enqueue hbs_cenc_subsamples on the current torch stream.  stream / index / nal_au / sub_first / sub / summary / keep /
        payload_off are device tensors (sub None: plan only; keep, payload_off may be None); params is an
        ndarray[CENC_PLAN_PARAMS] of one in host memory.  Returns the call's return code."""
        self._bind_stream()
        if sub_cap is None:
            sub_cap = _holds(sub, CENC_SUBSAMPLE.itemsize)
        params, params_p = _rec(params, CENC_PLAN_PARAMS)
        return self.lib.hbs_cenc_subsamples(self.h, _p(stream) if stream_bytes else None, int(stream_bytes), _p(index) if n_nals else None,
                                            int(n_nals), _p(keep), _p(nal_au) if n_nals else None, int(n_aus), _p(payload_off), params_p,
                                            _p(sub_first), _p(sub), int(sub_cap), _p(summary))

    def cenc_subsamples(self, stream, index, nal_au, n_aus, keep=None, payload_off=None, stream_bytes=None, **params):
        """Convenience: the subsample table of the samples hbs_mp4_fragment / hbs_annexb_to_lenpref make of `stream` (device
        uint8 tensor).  index / nal_au / keep / payload_off: host ndarrays or device tensors of their bytes; params: the
        keywords of cenc_plan_params.  Plans first, allocates the exact table, runs.  Returns (sub_first device tensor of
        (n_aus + 1) * 8 bytes, sub device tensor of the entries' bytes, summary record)."""
        name = "hbs_cenc_subsamples"
        d_idx, n = self._dv(index, NAL_ENTRY, empty=False)
        d_au, _ = self._dv(nal_au, np.uint32, empty=False)
        d_keep, _ = self._dv(keep, np.uint8)
        d_po, _ = self._dv(payload_off, np.uint64)
        nbytes = int(stream.numel()) if stream_bytes is None else int(stream_bytes)
        prm = cenc_plan_params(**params)
        summary = self._zeros()
        sub_first = self._empty((int(n_aus) + 1) * 8)
        args = (stream, nbytes, d_idx, n, d_au, n_aus, prm, sub_first)
        s = self._run(name, self.cenc_subsamples_async(*args, None, summary, keep=d_keep, payload_off=d_po), summary, " (NAL {0})")
        need = int(s["nal_count"])
        sub = self._empty(max(need, 2) * CENC_SUBSAMPLE.itemsize)
        s = self._run(name, self.cenc_subsamples_async(*args, sub, summary, keep=d_keep, payload_off=d_po, sub_cap=need), summary, " (NAL {0})")
        return sub_first, sub[: need * CENC_SUBSAMPLE.itemsize], s

    def cenc_crypt_async(self, data, data_bytes, sample_off, sample_size, n_samples, sub_first, sub, iv, params, summary):
        """Enqueue hbs_cenc_crypt on the current torch stream: AES-128-CTR in place over the protected ranges of the samples of
        `data`.  Everything but the counts and params (an ndarray[CENC_PARAMS] of one in host memory) is a device tensor; iv
        may be None with iv_mode 1.  Returns the call's return code."""
        self._bind_stream()
        params, params_p = _rec(params, CENC_PARAMS)
        on = bool(n_samples)
        return self.lib.hbs_cenc_crypt(self.h, _p(data) if data_bytes else None, int(data_bytes), _p(sample_off) if on else None,
                                       _p(sample_size) if on else None, int(n_samples), _p(sub_first) if on else None,
                                       _p(sub) if on else None, _p(iv), params_p, _p(summary))

    def cenc_crypt(self, data, sample_off, sample_size, sub_first, sub, key, iv=None, iv0=None, data_bytes=None):
        """Convenience: encrypts or decrypts (the same thing) the samples of `data` (device uint8 tensor) in place.  The four
        tables: host ndarrays (uint64, uint64, uint64, CENC_SUBSAMPLE) or device tensors of their bytes.  iv: n_samples x 16
        bytes (host or device), read; or iv0 (8 bytes): sequential IVs, and the blocks used are returned.  Returns (iv device
        tensor, summary record)."""
        name = "hbs_cenc_crypt"
        d_off, d_size, n = self._offsets_and_sizes(name, sample_off, sample_size, "sample")
        d_first, _ = self._dv(sub_first, np.uint64)
        d_sub, _ = self._dv(sub, CENC_SUBSAMPLE)
        d_iv, _ = self._dv(iv, np.uint8)
        if d_iv is None:
            d_iv = self._empty(max(n, 1) * 16)
        nbytes = int(data.numel()) if data_bytes is None else int(data_bytes)
        summary = self._zeros()
        prm = cenc_params(key, iv0=iv0 if iv is None else None)
        s = self._run(name, self.cenc_crypt_async(data, nbytes, d_off, d_size, n, d_first, d_sub, d_iv, prm, summary), summary, " (sample {0})")
        return d_iv[: n * 16], s

    def cbcs_crypt_async(self, data, data_bytes, sample_off, sample_size, n_samples, sub_first, sub, iv, params, summary):
        """Enqueue hbs_cbcs_crypt on the current torch stream: AES-128-CBC in place over the pattern of crypt blocks of the
        protected ranges of the samples of `data`; the direction is in params.  Everything but the counts and params (an
        ndarray[CBCS_PARAMS] of one in host memory) is a device tensor; iv may be None with iv_mode 1.  Returns the call's
        return code."""
        self._bind_stream()
        params, params_p = _rec(params, CBCS_PARAMS)
        on = bool(n_samples)
        return self.lib.hbs_cbcs_crypt(self.h, _p(data) if data_bytes else None, int(data_bytes), _p(sample_off) if on else None,
                                       _p(sample_size) if on else None, int(n_samples), _p(sub_first) if on else None,
                                       _p(sub) if on else None, _p(iv), params_p, _p(summary))

    def cbcs_crypt(self, data, sample_off, sample_size, sub_first, sub, key, iv=None, iv0=None, decrypt=False, crypt_byte_block=1,
                   skip_byte_block=9, whole_runs=False, data_bytes=None):
        """Convenience: encrypts (decrypt=True: decrypts) the samples of `data` (device uint8 tensor) in place, scheme cbcs.  The
        four tables: host ndarrays (uint64, uint64, uint64, CENC_SUBSAMPLE) or device tensors of their bytes.  iv: n_samples x
        16 bytes (host or device), or iv0: the constant 16-byte IV of every sample.  Returns the summary record."""
        name = "hbs_cbcs_crypt"
        d_off, d_size, n = self._offsets_and_sizes(name, sample_off, sample_size, "sample")
        d_first, _ = self._dv(sub_first, np.uint64)
        d_sub, _ = self._dv(sub, CENC_SUBSAMPLE)
        d_iv, _ = self._dv(iv, np.uint8)
        nbytes = int(data.numel()) if data_bytes is None else int(data_bytes)
        summary = self._zeros()
        prm = cbcs_params(key, iv0=iv0 if iv is None else None, flags=(CBCS_DECRYPT if decrypt else 0) | (CBCS_WHOLE_RUNS if whole_runs else 0),
                          crypt_byte_block=crypt_byte_block, skip_byte_block=skip_byte_block)
        return self._run(name, self.cbcs_crypt_async(data, nbytes, d_off, d_size, n, d_first, d_sub, d_iv, prm, summary), summary, " (sample {0})")

    def au_insert_async(self, stream, stream_bytes, index, parsed, n_nals, au, nal_au, n_aus, first_au, au_count, flags,
                        out, index_out, nal_src, nal_au_out, au_out, summary, out_cap=None, index_cap=0):
        """Enqueue hbs_au_insert on the current torch stream.  Everything but the counts and flags is a device tensor (out None:
        plan only; index_out, nal_src, nal_au_out, au_out may be None); index_cap: entries each per-NAL table has room for.
        Returns the call's return code (0, or HBS_E_ARG for arguments it refuses)."""
        self._bind_stream()
        if out_cap is None:
            out_cap = _holds(out)
        return self.lib.hbs_au_insert(self.h, _p(stream) if stream_bytes else None, int(stream_bytes), _p(index) if n_nals else None,
                                      _p(parsed) if n_nals else None, int(n_nals), _p(au) if n_aus else None,
                                      _p(nal_au) if n_aus and n_nals else None, int(n_aus), int(first_au), int(au_count), int(flags),
                                      _p(out), int(out_cap), _p(index_out), _p(nal_src), _p(nal_au_out), int(index_cap), _p(au_out), _p(summary))

    def au_insert(self, stream, index, parsed, n_nals, au, nal_au, first_au=0, au_count=None, flags=AUINS_AUD | AUINS_PARAM_SETS,
                  stream_bytes=None):
        """Convenience: AUDs and the parameter sets in force in front of the access units [first_au, first_au + au_count) of
        `stream` (device uint8 tensor).  index / parsed / au / nal_au: host ndarrays of the records or device tensors of them.
        Plans first, allocates the exact outputs, runs.  Returns (out, index_out, nal_src, nal_au_out, au_out, summary): device
        tensors (uint8 views of the records; int32 for the two number tables) cut to what was written, and the summary record."""
        name = "hbs_au_insert"
        t = self.torch
        au, n_aus = self._dv(au, ACCESS_UNIT)
        index, parsed, nal_au = (self._dv(x)[0] for x in (index, parsed, nal_au))
        if au_count is None:
            au_count = max(n_aus - first_au, 0)
        nbytes = int(stream.numel()) if stream_bytes is None else int(stream_bytes)
        summary = self._zeros()
        args = (stream, nbytes, index, parsed, n_nals, au, nal_au, n_aus, first_au, au_count, flags)
        s = self._run(name, self.au_insert_async(*args, None, None, None, None, None, summary), summary)
        need, m, r = int(s["stream_bytes"]), int(s["nal_count"]), int(s["reserved"][2])
        out = self._empty(max(need, 16))
        index_out = self._empty(max(m, 1) * NAL_ENTRY.itemsize)
        nal_src, nal_au_out = (t.empty(max(m, 1), dtype=t.int32, device=out.device) for _ in range(2))
        au_out = self._empty(max(r, 1) * ACCESS_UNIT.itemsize)
        s = self._run(name, self.au_insert_async(*args, out, index_out, nal_src, nal_au_out, au_out, summary, out_cap=need, index_cap=m), summary)
        return out[:need], index_out[: m * NAL_ENTRY.itemsize], nal_src[:m], nal_au_out[:m], au_out[: r * ACCESS_UNIT.itemsize], s

    def au_keep_async(self, nal_au, parsed, n_nals, first_au, au_count, keep, param_sets=False):
        """Enqueue hbs_au_keep: keep (device uint8 tensor of n_nals) becomes the mask hbs_filter_annexb takes as d_keep."""
        self._bind_stream()
        self._check(self.lib.hbs_au_keep(self.h, _p(nal_au), _p(parsed), int(n_nals), int(first_au), int(au_count),
                                         AUKEEP_PARAM_SETS if param_sets else 0, _p(keep)), "hbs_au_keep")

    def au_keep(self, nal_au, parsed, n_nals, first_au, au_count, param_sets=False):
        """-> device uint8 tensor of n_nals: 1 for the NALs of AUs [first_au, first_au + au_count) (and the parameter sets in force)"""
        keep = self._empty(max(n_nals, 1))
        self.au_keep_async(nal_au, parsed, n_nals, first_au, au_count, keep, param_sets)
        return keep[:n_nals]

