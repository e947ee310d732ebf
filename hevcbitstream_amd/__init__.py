"""hevcbitstream_amd -- MI355X (gfx950) Annex-B indexer / RBSP extractor.

Python is plumbing here: it loads the C-ABI library (include/hevcbitstream_amd.h,
built from csrc/*.hip by `make lib`) with ctypes and hands it device pointers of
torch tensors.  All work happens in the HIP kernels; there is no CPU fallback --
loading fails loudly when the library has not been built, and creating a
context fails when there is no gfx950 GPU."""
from .api import (Context, HbsError, NAL_ENTRY, PARSED, SUMMARY, ST_ERROR, ST_TRAILING03,  # noqa: F401
                  ST_UNTERMINATED, library_path, load_library, source_digest,
                  NAL_FILTER, NALMASK_VCL, NALMASK_IRAP, NALMASK_PARAM_SETS, NALMASK_SEI, NALMASK_ALL,
                  ACCESS_UNIT, AU_CARRY, AU_IRAP, AU_IDR, AU_CVS_START, AU_ANCHOR, AU_NO_PICTURE, AU_DAMAGED,
                  AU_PARAM_SETS, AU_END_OF_SEQ, AUKEEP_PARAM_SETS,
                  AU_TIMES_PARAMS, AUT_MAX_SPAN, AUT_DELAY_GIVEN, AUT_WRAP33, au_times_params,
                  CENC_SUBSAMPLE, CENC_PLAN_PARAMS, CENC_PARAMS, CENC_ALIGN16, CENC_SCHEME_CENC, cenc_plan_params, cenc_params,
                  CBCS_PARAMS, CBCS_DECRYPT, CBCS_WHOLE_RUNS, cbcs_params,
                  TS_PES, TS_PACKET, TS_FAULT, TS_OTHER, TS_SKIPPED, TS_NO_PAYLOAD, TS_PAYLOAD, TS_PES_START,
                  TS_F_PTS, TS_F_DTS, TS_F_RANDOM_ACCESS, TS_F_DISCONTINUITY, TS_F_DATA_ALIGNED, TS_NO_TIME,
                  STREAM_TYPE_HEVC, ts_packet, ts_find_pid,
                  TS_MUX_PARAMS, TSMUX_PCR, TSMUX_PSI_AT_IRAP, TSMUX_NO_PSI, ts_mux_params, ts_mux_psi, ts_mux_au_packets,
                  AUINS_AUD, AUINS_PARAM_SETS, AUINS_PARAM_SETS_FIRST, aud_nal,
                  RTP_PARAMS, RTP_PACKET, RTP_OPEN_END, RTP_AGGREGATE, RTP_AP_SPAN, RTP_SINGLE, RTP_FU, RTP_AP, RTP_OTHER,
                  rtp_params, rtp_nal_packets, rtp_packet, rtp_ap_units, rtp_packet_offsets,
                  RTP_UNPACK_PARAMS, RTPU_MATCH_SSRC, rtp_unpack_params, rtp_frames,
                  RTP_ORDER_PARAMS, RTPO_MATCH_SSRC, RTPO_AFTER, rtp_order_params,
                  MP4_PARAMS, MP4_FRAG, MP4_INIT_PARAMS, MP4_CUT_AT_IRAP, MP4_HEV1, mp4_params, mp4_fragment_bytes, mp4_init,
                  MP4_READ_PARAMS, MP4_TRACK, mp4_read_params, mp4_init_read,
                  MP4_STBL, MP4_STBL_CO64, mp4_stbl_find, mp4_track_read,
                  MP4_STBL_WRITE_PARAMS, mp4_stbl_write_params, mp4_stbl_write_bytes, mp4_moov,
                  MP4_PROTECT_PARAMS, MP4_TENC, MP4_SCHEME_CENC, MP4_SCHEME_CBCS, mp4_protect_params, mp4_protect_bytes, mp4_init_protect,
                  MP4_SENC_PARAMS, MP4_SENC_CLEAR_IF_ABSENT, mp4_senc_params, mp4_init_unprotect)

__all__ = ["Context", "HbsError", "NAL_ENTRY", "PARSED", "SUMMARY", "ST_ERROR", "ST_TRAILING03",
           "ST_UNTERMINATED", "library_path", "load_library", "source_digest",
           "NAL_FILTER", "NALMASK_VCL", "NALMASK_IRAP", "NALMASK_PARAM_SETS", "NALMASK_SEI", "NALMASK_ALL",
           "ACCESS_UNIT", "AU_CARRY", "AU_IRAP", "AU_IDR", "AU_CVS_START", "AU_ANCHOR", "AU_NO_PICTURE", "AU_DAMAGED",
           "AU_PARAM_SETS", "AU_END_OF_SEQ", "AUKEEP_PARAM_SETS",
           "AU_TIMES_PARAMS", "AUT_MAX_SPAN", "AUT_DELAY_GIVEN", "AUT_WRAP33", "au_times_params",
           "CENC_SUBSAMPLE", "CENC_PLAN_PARAMS", "CENC_PARAMS", "CENC_ALIGN16", "CENC_SCHEME_CENC", "cenc_plan_params", "cenc_params",
           "CBCS_PARAMS", "CBCS_DECRYPT", "CBCS_WHOLE_RUNS", "cbcs_params",
           "TS_PES", "TS_PACKET", "TS_FAULT", "TS_OTHER", "TS_SKIPPED", "TS_NO_PAYLOAD", "TS_PAYLOAD", "TS_PES_START",
           "TS_F_PTS", "TS_F_DTS", "TS_F_RANDOM_ACCESS", "TS_F_DISCONTINUITY", "TS_F_DATA_ALIGNED", "TS_NO_TIME",
           "STREAM_TYPE_HEVC", "ts_packet", "ts_find_pid",
           "TS_MUX_PARAMS", "TSMUX_PCR", "TSMUX_PSI_AT_IRAP", "TSMUX_NO_PSI", "ts_mux_params", "ts_mux_psi", "ts_mux_au_packets",
           "AUINS_AUD", "AUINS_PARAM_SETS", "AUINS_PARAM_SETS_FIRST", "aud_nal",
           "RTP_PARAMS", "RTP_PACKET", "RTP_OPEN_END", "RTP_AGGREGATE", "RTP_AP_SPAN", "RTP_SINGLE", "RTP_FU", "RTP_AP", "RTP_OTHER",
           "rtp_params", "rtp_nal_packets", "rtp_packet", "rtp_ap_units", "rtp_packet_offsets",
           "RTP_UNPACK_PARAMS", "RTPU_MATCH_SSRC", "rtp_unpack_params", "rtp_frames",
           "RTP_ORDER_PARAMS", "RTPO_MATCH_SSRC", "RTPO_AFTER", "rtp_order_params",
           "MP4_PARAMS", "MP4_FRAG", "MP4_INIT_PARAMS", "MP4_CUT_AT_IRAP", "MP4_HEV1", "mp4_params", "mp4_fragment_bytes", "mp4_init",
           "MP4_READ_PARAMS", "MP4_TRACK", "mp4_read_params", "mp4_init_read",
           "MP4_STBL", "MP4_STBL_CO64", "mp4_stbl_find", "mp4_track_read",
           "MP4_STBL_WRITE_PARAMS", "mp4_stbl_write_params", "mp4_stbl_write_bytes", "mp4_moov",
           "MP4_PROTECT_PARAMS", "MP4_TENC", "MP4_SCHEME_CENC", "MP4_SCHEME_CBCS", "mp4_protect_params", "mp4_protect_bytes", "mp4_init_protect",
           "MP4_SENC_PARAMS", "MP4_SENC_CLEAR_IF_ABSENT", "mp4_senc_params", "mp4_init_unprotect"]
