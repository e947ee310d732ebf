/*
 * hevcbitstream_amd.h -- batch C ABI of the MI355X (gfx950) Annex-B indexer /
 * RBSP extractor.  Plain C: pointers and sizes only, no C++/torch types.
 *
 * This is the 64-bit, whole-stream form of the reference's per-NAL byte layer:
 *
 *   hbs_index_extract   replaces the loop  find_nal_unit() + nal_to_rbsp()
 *                       reference: h264_nal.c:38-76 (find_nal_unit),
 *                       h264_nal.c:147-200 (nal_to_rbsp), driven as in
 *                       hevc_analyze.c:135-205 and hevc_stream.c:161-165
 *   hbs_emit_annexb     replaces  rbsp_to_nal() per NAL + start-code emission
 *                       reference: h264_nal.c:92-132, hevc_stream.c:1324-1327
 *   hbs_parse_headers   replaces  read_hevc_nal_unit() per NAL
 *                       reference: hevc_stream.c:155-240 and the readers it
 *                       dispatches to (:243-1218)
 *   hbs_index_parse     find_nal_unit over the stream + read_hevc_nal_unit per NAL without
 *                       an RBSP arena (each header is stripped from the stream by itself)
 *   hbs_parse_headers_trace   the same with the per-field trace read_debug_hevc_nal_unit
 *                       prints (hevc_stream.c:2343-3434)
 *   hbs_write_headers   replaces  write_hevc_nal_unit() per NAL up to rbsp_to_nal
 *                       reference: hevc_stream.c:1249-1327 and the writers behind it
 *   hbs_index_extract_host    hbs_index_extract for a stream in HOST memory of any
 *                       length, windowed (replaces the reader of hevc_analyze.c:124-210)
 *   hbs_synth_*         synthetic stream S(seed, n_nals, mode) of SURVEY.md
 *                       8(d) (no reference counterpart: it ships no streams)
 *
 * All `d_` pointers are DEVICE pointers of the context's GPU (hipMalloc'ed or
 * torch-allocated), 16-byte aligned -- anywhere inside an allocation: a buffer
 * need not begin one, nothing in front of or behind a buffer is written, and no
 * byte outside an input decides a result.  Where an entry point takes less it
 * says so ("Alignment:" in its comment; tests/test_gpu_carved.py runs each call
 * at every alignment stated); a pointer below the stated alignment is refused
 * with HBS_E_ARG before anything is written.  Calls enqueue work on the context's HIP
 * stream and return without synchronising unless stated otherwise.  Return
 * value: 0 on success, a negative HBS_E_* code otherwise.  There is no CPU
 * fallback: without a usable gfx950 device every call fails with
 * HBS_E_NO_DEVICE.
 *
 * The legacy single-NAL symbols of the reference (find_nal_unit, nal_to_rbsp,
 * rbsp_to_nal, read_hevc_nal_unit, ...) are declared in h264_stream.h /
 * hevc_stream.h next to this file and are thin host wrappers over this API.
 */
#ifndef HEVCBITSTREAM_AMD_H
#define HEVCBITSTREAM_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HBS_E_NO_DEVICE   (-1)   /* no gfx950 GPU / HIP runtime failure at init  */
#define HBS_E_HIP         (-2)   /* a HIP call failed (see hbs_last_error)       */
#define HBS_E_ARG         (-3)   /* bad argument (alignment, null, capacity 0)   */
#define HBS_E_CAPACITY    (-4)   /* index / arena / output capacity too small    */
#define HBS_E_TIMEOUT     (-5)   /* in-kernel look-back wait gave up (bug guard) */
#define HBS_E_DEPTH       (-6)   /* hbs_parse_headers_compact / _materialize on an out-of-spec stream whose answer needs the
                                    sequential parse (a chain of slice-own RPS sets deeper than 3): take hbs_parse_headers;
                                    hbs_au_times on a table that reorders an AU across more than HBS_AUT_MAX_SPAN others */

/* per-NAL status flags */
#define HBS_ST_ERROR        1    /* nal_to_rbsp() would return -1 (h264_nal.c:156-167) */
#define HBS_ST_TRAILING03   2    /* NAL ends in 00 00 03: the 03 is dropped and
                                    nal_to_rbsp() consumes len-1 (h264_nal.c:170-173) */
#define HBS_ST_UNTERMINATED 4    /* last NAL: find_nal_unit() returned -1 with
                                    nal_end = size (h264_nal.c:71)                */

/* One NAL of the whole-stream index: what find_nal_unit() reports for it when
 * the stream is walked as in hevc_analyze.c:135-205, with 64-bit offsets, plus
 * where nal_to_rbsp() of it went. 32 bytes. */
typedef struct hbs_nal_entry {
    uint64_t start;      /* offset of the first payload byte (after 00 00 01)   */
    uint64_t end;        /* offset one past the last payload byte               */
    uint64_t rbsp_off;   /* offset of this NAL's RBSP in the RBSP arena         */
    uint32_t rbsp_len;   /* RBSP bytes = (end-start) - emulation-prevention bytes */
    int32_t  status;     /* HBS_ST_* flags                                      */
} hbs_nal_entry;

/* Result block of hbs_index_extract (written on the DEVICE; copy it with
 * hbs_read_summary). */
typedef struct hbs_summary {
    uint64_t nal_count;     /* NALs in the index (what the reference loop visits) */
    uint64_t nal_found;     /* start codes found before truncation/capacity clip  */
    uint64_t rbsp_bytes;    /* bytes written to the RBSP arena                    */
    uint64_t stream_bytes;  /* bytes scanned                                      */
    int32_t  stop_reason;   /* 0: no more start codes; -1: last NAL unterminated;
                               1: stopped at an empty NAL (find_nal_unit == 0 with
                               a start code found, hevc_analyze.c:135)            */
    int32_t  error;         /* 0 or HBS_E_CAPACITY / HBS_E_TIMEOUT / HBS_E_ARG    */
    uint64_t reserved[3];
} hbs_summary;

typedef struct hbs_ctx hbs_ctx;

/* Create a context on HIP device `device` (one per GPU / per rank).
 *
 * Threads and streams.  A context owns ONE set of scratch on its GPU (run header, look-back words, ticket, the workspaces of
 * K3 / K4 / K5, the window buffers of hbs_index_extract_host) and binds to ONE stream at a time, so:
 *   - a context is used by one thread at a time (the library takes no lock in the batch API: callers that share a
 *     context serialise their calls themselves);
 *   - DIFFERENT contexts are independent: any number of threads, one context each, may call at the same time on the
 *     same or on different GPUs (tests/test_gpu_legacy.py::test_batch_api_two_contexts_two_threads);
 *   - all work of a context is ordered by the stream it is bound to when the call is made.  Re-binding the stream
 *     (hbs_ctx_set_stream) while work enqueued through the previous one may still be running is the caller's to order
 *     (an event between the two streams): the scratch is shared by both.  hbs_index_extract_host uses two private streams
 *     and returns only when they are idle.
 * The legacy single-NAL symbols (find_nal_unit ... write_hevc_nal_unit) share one internal context behind a process-wide
 * lock: safe from any thread, serialised (hbs_legacy.c).
 *
 * HIP graphs.  These calls only enqueue -- no host wait, no allocation once the scratch has its size, every choice that depends
 * on the data made on the device -- and may be captured into a HIP graph (hipStreamBeginCapture on the bound stream) after ONE
 * warm-up call with the same arguments, which sizes the scratch, and replayed on other contents of the same buffers:
 *   hbs_index_extract, hbs_emit_annexb, hbs_parse_headers, hbs_parse_extended, hbs_filter_annexb, hbs_annexb_to_lenpref,
 *   hbs_lenpref_to_annexb, hbs_ts_demux, hbs_ts_mux, hbs_au_insert, hbs_au_keep, hbs_rtp_pack (with and without
 *   HBS_RTP_AGGREGATE), hbs_rtp_unpack, hbs_rtp_order, hbs_mp4_fragment, hbs_mp4_samples,
 *   hbs_mp4_stbl_samples, hbs_mp4_stbl_write, hbs_au_times, hbs_cenc_subsamples, hbs_cenc_crypt,
 *   hbs_cbcs_crypt, hbs_mp4_protect, hbs_mp4_senc_samples.
 * hbs_cenc_crypt takes its key and iv0 from host memory when it is called: a captured graph replays with the key and iv0 it was
 * captured with.  So does hbs_cbcs_crypt, and with the direction and the pattern of the capture.
 * The list is what tests/test_gpu_graphs.py, tests/test_gpu_scan.py, tests/test_gpu_rtp.py, tests/test_gpu_rtp_ap.py,
 * tests/test_gpu_rtp_unpack.py, tests/test_gpu_rtp_order.py, tests/test_gpu_mp4.py, tests/test_gpu_mp4_read.py,
 * tests/test_gpu_mp4_stbl.py, tests/test_gpu_mp4_stbl_write.py, tests/test_gpu_au_times.py, tests/test_gpu_cenc.py and
 * tests/test_gpu_cbcs.py and tests/test_gpu_mp4_protect.py and tests/test_gpu_mp4_senc.py replay, no more: hbs_parse_headers_compact,
 * hbs_parse_materialize, hbs_write_headers and hbs_access_units do not wait either, but no test has replayed them, and three
 * of the calls above were wrong at a replay until one did -- capture them at your own risk.
 * A replay is the captured call on what the buffers hold then: every argument the host passed (counts, byte sizes, capacities,
 * flags, params, `initial` records) keeps the value it had at capture, so a graph serves inputs that agree in all of them, and a
 * capture must not need the scratch to grow.  Timing stays off during a capture (hbs_ctx_enable_timing records events and keeps
 * host state per call).
 * The calls that wait for the device, and therefore are never captured: hbs_index_parse*, hbs_index_extract_host, hbs_gather_*,
 * hbs_trim_part, hbs_read_summary, hbs_ctx_last_kernel, hbs_ctx_last_emit_by_tiles, hbs_ctx_kernel_ms*, hbs_ctx_synchronize
 * and the synchronous copies (hbs_copy_to_device, hbs_copy_to_host).  After a replay hbs_ctx_last_kernel and
 * hbs_ctx_last_emit_by_tiles speak of that replay: both read what the device left, at every call of them. */
int  hbs_ctx_create(hbs_ctx** out, int device);
void hbs_ctx_destroy(hbs_ctx* ctx);
/* A new context enqueues on a non-blocking stream of its own.  set_stream
 * makes it use the caller's HIP stream instead (hipStream_t passed as void*;
 * NULL = the HIP null stream); use_own_stream goes back. */
int  hbs_ctx_set_stream(hbs_ctx* ctx, void* hip_stream);
int  hbs_ctx_use_own_stream(hbs_ctx* ctx);
void* hbs_ctx_get_stream(hbs_ctx* ctx);
int  hbs_ctx_synchronize(hbs_ctx* ctx);
/* Measurement aid: when enabled, hbs_index_extract records HIP events on the
 * context's stream around its dominant kernel (the fused scan/extract kernel)
 * only (for an index-only call: its four kernels); hbs_ctx_kernel_ms waits for the
 * last such launch and returns its duration, hbs_ctx_kernel_ms_back(back) that of the
 * call `back` calls earlier (the event pairs of the last 64 timed calls are kept, so a
 * benchmark can read every step of its timed loop after the loop, without a wait
 * inside it).  hbs_ctx_grid reports the persistent grid used. */
int  hbs_ctx_enable_timing(hbs_ctx* ctx, int on);
int  hbs_ctx_kernel_ms(hbs_ctx* ctx, float* ms);
int  hbs_ctx_kernel_ms_back(hbs_ctx* ctx, int back, float* ms);
int  hbs_ctx_grid(hbs_ctx* ctx, int* blocks, int* blocks_per_cu);
/* The scan + extract kernels are persistent and fill the GPU: a kernel of another stream (RCCL's, in hbs_gather_index running
 * beside the next scan) finds no CU before the scan ends.  `spare` workgroup slots are left free from now on (0 = none, the
 * default; a multi-GPU caller that overlaps the index gather with the next scan wants ~32 of the 512: with 8 or 16 RCCL still
 * waited for the scan to end, with 32 a one-rank gather of 54 MB took 0.14 ms beside the scan instead of 5.3 ms behind it).
 * Covers every scan kernel: the register-tile and LDS-image kernels launch `spare` workgroups fewer, the index-only streaming
 * kernel 4 x `spare` one-wavefront workgroups fewer.  An HBS_GRID_BLOCKS debugging cap stays a ceiling of its own. */
int  hbs_ctx_reserve_workgroups(hbs_ctx* ctx, int spare);
/* Tile hand-out of the persistent kernels (scan + extraction, arena-tile emit).  Default (0): every tile by atomic ticket, in
 * arrival order -- a workgroup's look-back only ever waits for tiles that a RUNNING workgroup has claimed, so calls of several
 * contexts or processes may share a device.  on = 1: the caller states that while this context's calls run, no other persistent
 * kernel uses the device; a workgroup's first tile is then its own number (later ones by ticket), which saves the start-of-call
 * queue on the ticket word (~1 % of a 1 GiB call, nothing at 16 GiB).  With static first tiles, forward progress assumes every
 * workgroup of the grid is resident at once: do NOT set it when two contexts (or ranks) scan one device concurrently. */
int  hbs_ctx_set_device_exclusive(hbs_ctx* ctx, int on);
/* Implementations of the scan kernel, with identical results:
 * 4 = event-sparse, tile held in registers: 48 rows of 1 KiB per wavefront, 192 KiB tiles, up to 512 candidate chunks a tile
 *     (hbs_scan4.hip; the fastest on coded video, where zero pairs are rare, and the slowest on zero-heavy data),
 * 6 = the same kernel with 24 rows per wavefront: 96 KiB tiles, up to 1024 candidate chunks a tile, all four wavefronts on them
 *     (hbs_scan4_r24.hip, round 6; streams that are dense but regular -- NALs of ~120 to ~450 bytes --, with or without an arena),
 * 2 = tile staged in an LDS image (hbs_scan.hip; same speed on any data),
 * 5 = index only (no RBSP arena asked for): nothing has to stay in registers, so the bytes are
 *     streamed and only the flagged chunks are looked at again (hbs_scan5.hip); with an arena it means 4,
 * 0 = automatic, the default: a density probe (64 windows of 16 KiB) runs in front and the kernel is picked from it on the
 *     device, without a host round trip: 4 up to one candidate chunk in 44, 6 up to one in 6.5, 2 beyond; when no arena is asked
 *     for and the stream is 1 GiB or more: 5 up to one in 9, 2 beyond.
 * Environment HBS_KERNEL=0|2|4|5|6 sets the default.  hbs_ctx_last_kernel waits for the last
 * hbs_index_extract and says which kernel ran it. */
int  hbs_ctx_set_kernel(hbs_ctx* ctx, int variant);
int  hbs_ctx_get_kernel(hbs_ctx* ctx);
/* Kernel 4 walks a DENSE tile (one with more than 512 candidate chunks in its 192 KiB: padding, zero stuffing) chunk by chunk,
 * and every tile behind it waits for its count.  From round 5 such tiles are counted AHEAD of the main kernel: the call's first
 * launch samples every tile, a small kernel counts the ones the sample marks, and the main kernel takes those counts instead of
 * walking the tile a first time (hbs_scan4.hip, "dense tiles counted ahead").  mode 1 (default): streams of 3 GiB and more;
 * 0: never; 2: any stream that has more than one tile.  Results are identical in all three.  Environment HBS_COUNT_AHEAD=0|1|2
 * sets the default.  The table costs 76 bytes of device memory per 192 KiB of stream; nothing of it lives on the host, so a call captured into a HIP graph may be replayed.
 * The table is allocated by the first call that needs it (and again by a call on a longer stream): such a call must not be made
 * inside a stream capture -- make one call of at least that size before capturing (round 5's advice).
 * Since round 6 the same mode governs hbs_emit_annexb's arena-tile kernel, which samples the arena and counts the dense tiles it
 * lists ahead in the same way (two launches in front of the main pass): mode 1 = arenas of 3 GiB and more. */
int  hbs_ctx_set_count_ahead(hbs_ctx* ctx, int mode);
int  hbs_ctx_last_kernel(hbs_ctx* ctx);
/* Text of the last HIP/driver error seen by this context. */
const char* hbs_last_error(hbs_ctx* ctx);
/* Library/self description: "hevcbitstream_amd <ver> gfx950 ..." */
const char* hbs_version(void);

/*
 * Start-code scan + NAL index + RBSP extraction over one stream resident in
 * HBM (single pass: every stream byte is read once, every RBSP byte written
 * once).
 *
 *   d_stream, stream_bytes   Annex-B bytes
 *   d_index, index_cap       out: hbs_nal_entry[index_cap]; the call zeroes it
 *   d_rbsp, rbsp_cap         out: packed RBSP arena (NAL k at rbsp_off, rbsp_len);
 *                            NULL = index only (rbsp_off/rbsp_len still filled)
 *   d_summary                out: hbs_summary on the device
 *
 * Semantics (bit-exact with the reference on the same bytes):
 *   - entries are the NALs the loop `while (find_nal_unit(p, sz, &s, &e) > 0)`
 *     of hevc_analyze.c:135-177 visits over the whole stream, followed by the
 *     "last NAL" of the -1 path (:190-205), offsets relative to d_stream;
 *   - RBSP of NAL k is what nal_to_rbsp() writes for it; for a NAL it rejects
 *     (HBS_ST_ERROR) the arena holds every byte except 00 00 03 emulation
 *     bytes (the reference leaves its output unspecified there);
 *   - bytes past the end of the stream are taken as 0xFF where the reference
 *     reads them unchecked (h264_nal.c:47-48, 65-66).
 * Alignment: d_stream, d_rbsp, d_summary 16 bytes; d_index 8 bytes.
 */
int hbs_index_extract(hbs_ctx* ctx,
                      const uint8_t* d_stream, uint64_t stream_bytes,
                      hbs_nal_entry* d_index, uint64_t index_cap,
                      uint8_t* d_rbsp, uint64_t rbsp_cap,
                      hbs_summary* d_summary);

/*
 * The same for a stream in HOST memory of any length (larger than device memory is fine): the
 * stream is uploaded window by window (window_bytes each, >= 4096, rounded down to 16), the
 * upload of one window overlapping the scan and the download of the previous one; index and RBSP
 * arrive in host memory with offsets relative to h_stream / h_rbsp, identical to what
 * hbs_index_extract returns for the whole stream.  Replaces the windowed reader of
 * hevc_analyze.c:124-210 (and gets a NAL that straddles two reads right).
 * A NAL (with the zeros in front of it) that does not fit the window makes the window GROW (round 5): the walk goes on from
 * the end of the last complete NAL with device windows of twice the size, as often as it takes, up to the ceiling set with
 * hbs_ctx_set_ingest_window_max (default 1 GiB; a ceiling at or below window_bytes: no growth); h_summary->reserved[0] = the
 * window size the call ended with (0: never grown).  Past the ceiling: HBS_E_CAPACITY in h_summary->error, reserved[2] = 1
 * and reserved[1] = the stream offset of the NAL that did not fit -- everything in front of it has been delivered.  (The
 * reference's fixed 32 MiB reader parses such a NAL cut short, hevc_analyze.c:126,190-209.)  A window must not hold more than
 * window_bytes/16 NALs (HBS_E_CAPACITY otherwise).  Page-locked host buffers make the transfers asynchronous; pageable ones work.
 */
int hbs_index_extract_host(hbs_ctx* ctx, const uint8_t* h_stream, uint64_t stream_bytes, uint64_t window_bytes,
                           hbs_nal_entry* h_index, uint64_t index_cap,
                           uint8_t* h_rbsp, uint64_t rbsp_cap, hbs_summary* h_summary);
/* Device memory: a window of W bytes holds two stream buffers of 2 W, an RBSP buffer of 2 W (when h_rbsp is asked for) and an
 * index of 2 W / 32 entries -- about 8 W in all; every growth step frees them and allocates the next size, so at the default
 * ceiling a call may hold ~8 GiB on the device.  Lower the ceiling where that is too much.  When the call returns a hard error
 * (non-zero return value) h_summary still says what the runs before the failing one delivered (nal_count, rbsp_bytes). */
int hbs_ctx_set_ingest_window_max(hbs_ctx* ctx, uint64_t max_window_bytes /* 0: the default, 1 GiB */);

/*
 * K3: re-emit Annex-B from an RBSP arena: for every NAL, the bytes between the
 * previous NAL and this one (zeros and the 01 of the start code) followed by
 * rbsp_to_nal() of its RBSP (h264_nal.c:92-132: a 03 is inserted in front of
 * any byte <= 3 that follows two zeros; nothing is appended after a trailing
 * 00 00).
 *
 *   d_rbsp, rbsp_bytes                the arena and its size: nothing at or behind d_rbsp + rbsp_bytes
 *                                     is read -- an entry with rbsp_off + rbsp_len > rbsp_bytes ends the
 *                                     call with HBS_E_ARG in the summary before any byte is read through
 *                                     the index -- and the NALs must add up to at most rbsp_bytes
 *                                     (they do unless entries overlap; else HBS_E_CAPACITY)
 *   d_index_in[k].rbsp_off/rbsp_len   where NAL k's RBSP lives in d_rbsp
 *   gap_mode 0   gap of NAL k = d_index_in[k].start - d_index_in[k-1].end
 *                (start of NAL 0 for k = 0): what hbs_index_extract recorded
 *   gap_mode 1   synthetic rule: 00 00 00 01 when k % 4 == 0, else 00 00 01
 *   d_index_out  (optional) entries with start/end in the emitted stream
 *   d_summary    stream_bytes = bytes emitted; error = HBS_E_CAPACITY if
 *                out_cap was too small.  hbs_annexb_bound(rbsp_bytes, n_nals) is always enough for
 *                gap_mode 1; with gap_mode 0 the recorded gaps (zero bytes between NALs, any number
 *                of them) come on top: hbs_annexb_bound_gaps(rbsp_bytes, n_nals, gap_bytes) with
 *                gap_bytes = the sum of the gaps -- at most the `start` of the last entry of the
 *                index the gaps are taken from
 *
 * Emitting what hbs_index_extract extracted reproduces the input stream byte
 * for byte when every NAL was accepted (no HBS_ST_ERROR), none ended in
 * 00 00 03 (HBS_ST_TRAILING03: the reference drops that byte for good), the
 * bytes between NALs were zeros + 01, and the stream ends with its last NAL.
 * Alignment: d_rbsp and d_out any byte; d_index_in, d_index_out 8 bytes; d_summary 16 bytes.
 */
int hbs_emit_annexb(hbs_ctx* ctx, const uint8_t* d_rbsp, uint64_t rbsp_bytes,
                    const hbs_nal_entry* d_index_in, uint64_t n_nals, int gap_mode,
                    uint8_t* d_out, uint64_t out_cap, hbs_nal_entry* d_index_out, hbs_summary* d_summary);
uint64_t hbs_annexb_bound(uint64_t rbsp_bytes, uint64_t n_nals);
uint64_t hbs_annexb_bound_gaps(uint64_t rbsp_bytes, uint64_t n_nals, uint64_t gap_bytes);

/*
 * Cut an Annex-B stream down to some of its NAL units (keyframes only, temporal sub-layer extraction, stripping AUD / SEI /
 * filler before muxing), on the device, with the index hbs_index_extract / hbs_index_parse made of it.
 *
 *   rule        HOST pointer: which NAL units pass, by the two header bytes stream[start], stream[start + 1] read raw
 *               (nal_unit_type = (b0 >> 1) & 63, nuh_layer_id = ((b0 & 1) << 5) | (b1 >> 3), nuh_temporal_id_plus1 = b1 & 7:
 *               the fields hbs_parse_headers reports; the forbidden bit and the status flags play no part).  A NAL passes iff
 *               bit nal_unit_type of keep_types is set, nuh_temporal_id_plus1 <= max_temporal_id_plus1 and
 *               nuh_layer_id <= max_layer_id; a NAL with end - start < 2 has no header and passes iff keep_short != 0.
 *   d_keep      instead of a rule: n_nals bytes on the device, non-zero = keep.  Exactly one of rule and d_keep is non-NULL.
 *   d_out       the output (16-byte aligned); NULL = plan only: only d_summary is written, stream_bytes = the output's size
 *   d_index_out optional: room for n_nals entries
 *
 * The unit of NAL k is the stream bytes [end_{k-1}, end_k) (end_{-1} = 0): the zeros, the start code and whatever the start
 * search skipped in front of the NAL, then its payload, all verbatim.  The output is the units of the kept NALs in index order,
 * back to back (a rule that keeps everything writes stream[0, end_{n-1})).  d_index_out[j] describes the j-th kept NAL: start
 * and end as offsets in the output, rbsp_len copied, rbsp_off the running sum of the kept rbsp_len, status the input status
 * with HBS_ST_UNTERMINATED cleared and then set on the last kept entry only.  That is what hbs_index_extract of the output
 * returns, with one exception: find_nal_unit's `i+4 >= size` rule (h264_nal.c:52) does not find a last kept NAL whose start
 * code does not begin its unit and whose payload is short -- fewer than 2 bytes behind a 3-byte code (00 00 01), none behind a
 * 4-byte one (00 00 00 01) -- so the scan of the output ends one NAL earlier.
 *
 * d_summary: nal_count = kept NALs, nal_found = n_nals, rbsp_bytes = sum of the kept rbsp_len, stream_bytes = output bytes,
 * stop_reason = -1 if anything was kept, else 0.  error = HBS_E_ARG when the index is inconsistent (start > end,
 * end > stream_bytes or start_k < end_{k-1}; each entry is checked before its header bytes are read), HBS_E_CAPACITY when
 * out_cap is smaller than the output; in both cases nothing is written to d_out or d_index_out.  n_nals = 0 is valid (empty
 * output).  Nothing outside [d_out, d_out + output bytes) is stored, and no load touches a 16-byte granule that holds no byte
 * of the stream.  Returns HBS_E_ARG at once on bad arguments (both or neither of rule / d_keep, misaligned pointers).
 * Alignment: d_stream, d_out, d_summary 16 bytes; d_index, d_index_out 8 bytes; d_keep any byte.
 */
typedef struct hbs_nal_filter {
    uint64_t keep_types;             /* bit t set: NAL units with nal_unit_type t pass                                   */
    int32_t  max_temporal_id_plus1;  /* pass iff nuh_temporal_id_plus1 <= this (7: no limit; 0 in the header passes)     */
    int32_t  max_layer_id;           /* pass iff nuh_layer_id <= this (63: no limit)                                     */
    int32_t  keep_short;             /* NAL units with end - start < 2 have no header: kept iff non-zero                 */
    int32_t  reserved;               /* 0                                                                                */
} hbs_nal_filter;                    /* 24 bytes */

#define HBS_NALMASK_VCL        0x00000000FFFFFFFFull    /* types 0..31                */
#define HBS_NALMASK_IRAP       0x0000000000FF0000ull    /* types 16..23               */
#define HBS_NALMASK_PARAM_SETS 0x0000000700000000ull    /* types 32..34: VPS SPS PPS  */
#define HBS_NALMASK_SEI        0x0000018000000000ull    /* types 39, 40               */

int hbs_filter_annexb(hbs_ctx* ctx, const uint8_t* d_stream, uint64_t stream_bytes,
                      const hbs_nal_entry* d_index, uint64_t n_nals,
                      const hbs_nal_filter* rule, const uint8_t* d_keep,
                      uint8_t* d_out, uint64_t out_cap,
                      hbs_nal_entry* d_index_out, hbs_summary* d_summary);

/*
 * Length-prefixed NAL units: the framing of an MP4 / ISOBMFF `hvc1` sample (ISO/IEC 14496-15), of Matroska and of RTP
 * aggregation.  Each NAL unit is a RECORD: a big-endian length field of L = length_size bytes (1, 2 or 4: lengthSizeMinusOne
 * + 1 of hvcC) followed by that many payload bytes; a SAMPLE is one access unit's records back to back.  The two calls convert
 * between this and Annex-B on the device.  Throughout, any other length_size returns HBS_E_ARG at once.
 *
 * hbs_annexb_to_lenpref: Annex-B stream + index (+ keep mask, + the AU number of every NAL) -> records (+ sample table).
 *
 *   d_keep        n_nals bytes, non-zero = keep (hbs_au_keep writes this); NULL: every NAL is kept
 *   d_nal_au      optional: n_nals AU numbers, as hbs_access_units wrote them; n_aus = its AU count.  NULL: no sample table
 *                 (n_aus and d_sample_off are ignored)
 *   d_sample_off  with d_nal_au: n_aus + 1 offsets (optional even then: the AU table is checked either way)
 *   d_out         the output; NULL = plan only: only d_summary is written, stream_bytes = the output's size
 *   d_index_out   optional: room for n_nals entries
 *
 * The output is the records of the kept NALs in index order, back to back.  The record of NAL k is L bytes holding
 * end_k - start_k big-endian, then stream[start_k, end_k) verbatim; a kept NAL with end == start is a record of L zero bytes.
 * Nothing between NALs (zeros, start codes, junk) is copied.  d_index_out[j] describes the j-th kept NAL: start and end are
 * its payload's offsets in the output (behind the length field), rbsp_len is copied, rbsp_off is the running sum of the kept
 * rbsp_len, status is the input status with HBS_ST_UNTERMINATED cleared.
 * Sample table: d_sample_off[a], a = 0 .. n_aus, is the sum of the record bytes of the kept NALs k with d_nal_au[k] < a, so
 * sample a is out[d_sample_off[a], d_sample_off[a + 1]) and an AU with nothing kept is an empty sample.  The AU numbers are
 * checked, not trusted: d_nal_au[0] == 0, each step d_nal_au[k] - d_nal_au[k-1] is 0 or 1, d_nal_au[n_nals-1] == n_aus - 1;
 * with n_nals == 0, n_aus must be 0.
 * d_summary: nal_count = kept NALs, nal_found = n_nals, rbsp_bytes = sum of the kept rbsp_len, stream_bytes = output bytes,
 * stop_reason = 0, reserved = 0.  error = HBS_E_ARG when the index is inconsistent by hbs_filter_annexb's definition
 * (start > end, end > stream_bytes or start_k < end_{k-1}; each entry is checked before it is used), when a kept NAL has
 * end - start > 2^(8 L) - 1, or when the AU numbers break a rule above; else HBS_E_CAPACITY when out_cap is smaller than the
 * output (the sizes in the summary are right then; with HBS_E_ARG nal_count, rbsp_bytes and stream_bytes mean nothing).  On
 * either error nothing is written to d_out, d_index_out or d_sample_off.  n_nals = 0 is valid (empty output, d_sample_off[0] = 0).
 * Nothing outside [d_out, d_out + output bytes) is stored, no load touches a 16-byte granule that holds no byte of the
 * stream, and the call does not synchronise with the host.
 * Alignment: d_stream, d_out, d_summary 16 bytes; d_index, d_index_out, d_sample_off 8 bytes; d_nal_au 4 bytes; d_keep any byte.
 *
 * hbs_lenpref_to_annexb: samples of records anywhere in a buffer -> one Annex-B stream.
 *
 *   d_sample_off / d_sample_size   n_samples each: sample s is d_in[off_s, off_s + size_s).  Samples may lie anywhere in the
 *                 buffer, in any order, overlap, and have other data between them (an mdat with interleaved tracks)
 *   startcode_bytes   3: 00 00 01, 4: 00 00 00 01 in front of every NAL unit (anything else: HBS_E_ARG at once)
 *   nal_cap       the most records the call may find: with out_cap it sizes the scratch, as index_cap does elsewhere
 *   d_out         the output; NULL = plan only: only d_summary is written (and nal_cap and out_cap size nothing)
 *   out_cap       bytes of room at d_out.  It sizes the copy's grid and the scratch -- 8 bytes a 64 KiB of out_cap, 16 bytes a
 *                 record for min(nal_cap, out_cap / startcode_bytes) records -- so pass what the plan gave, not "plenty";
 *                 with d_out, an out_cap above 2^46 is refused with HBS_E_ARG at once (nal_cap may be anything, UINT64_MAX
 *                 for "no limit" included)
 *   d_sample_off_out  optional: n_samples + 1 offsets
 *
 * A sample is a chain of records: at p, L bytes of big-endian length n, then n payload bytes, then the next record at
 * p + L + n, until p reaches the sample's end.  The output is, for every sample in table order and every record in chain
 * order, the start code and then the payload; a zero-length record gives a bare start code.  d_sample_off_out[s] = the output
 * offset where sample s begins, entry n_samples the total.  No index is produced: run hbs_index_extract on the output.
 * Scanning it (find_nal_unit's walk) finds exactly the payloads, in order, as long as no payload but the last ends in 00 and
 * none holds 00 00 00 or 00 00 01 -- which holds for payloads that such a walk found (a found payload never ends in 00 unless
 * it is the stream's last, so the start code behind it cannot shorten it).  One exception, at the output's end: a last record
 * of length 0 behind a 3-byte start code, with a record in front of it, is not found, and the payload in front of it comes out
 * three bytes longer (the walk's `i+3 >= size` rule ends it at the buffer's end before the last start code is looked at).
 * A walk does yield such an index: a stream that ends in 00 00 00 01 behind a NAL has an empty last NAL; 4-byte codes keep it.
 * d_summary: nal_count = records, nal_found = n_samples, stream_bytes = output bytes, rbsp_bytes = 0, stop_reason = -1 if
 * nal_count > 0, else 0.  error = HBS_E_ARG when a sample leaves the buffer (off + size > in_bytes, or the sum wraps) or a
 * chain is malformed (fewer than L bytes left in front of the sample's end, or a length larger than what is left); then
 * reserved[0] = 1 + the lowest such sample (0 otherwise), and nal_count / stream_bytes count the well-formed records in front
 * of each sample's end or fault (none for a sample that leaves the buffer).  Else error = HBS_E_CAPACITY when
 * nal_count > nal_cap or out_cap is smaller than the output; the counts are right.  On an error nothing is written to d_out
 * or d_sample_off_out.  n_samples = 0 is valid.
 * The chain is the one sequential thing here and it is per sample: one lane walks one sample (twice: to count, and to place
 * once the offsets are known), so a single sample with very many records is walked by one lane, at the latency of one
 * dependent load a record.
 * The same store and load guarantees as above (loads: 16-byte granules that hold a byte of d_in[0, in_bytes)); no host
 * synchronisation.  Alignment: d_in, d_out, d_summary 16 bytes; d_sample_off, d_sample_size, d_sample_off_out 8 bytes.
 */
int hbs_annexb_to_lenpref(hbs_ctx* ctx, const uint8_t* d_stream, uint64_t stream_bytes,
                          const hbs_nal_entry* d_index, uint64_t n_nals,
                          const uint8_t* d_keep /* n_nals bytes, non-zero = keep; NULL: all */,
                          int length_size,
                          const uint32_t* d_nal_au /* optional: AU number per NAL, as hbs_access_units wrote it */,
                          uint64_t n_aus, uint64_t* d_sample_off /* n_aus + 1, with d_nal_au */,
                          uint8_t* d_out, uint64_t out_cap,
                          hbs_nal_entry* d_index_out /* optional, n_nals entries */, hbs_summary* d_summary);
int hbs_lenpref_to_annexb(hbs_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes, int length_size,
                          const uint64_t* d_sample_off, const uint64_t* d_sample_size, uint64_t n_samples,
                          int startcode_bytes /* 3: 00 00 01, 4: 00 00 00 01 */, uint64_t nal_cap,
                          uint8_t* d_out, uint64_t out_cap,
                          uint64_t* d_sample_off_out /* optional, n_samples + 1 */, hbs_summary* d_summary);

/*
 * ---- access units -> fragmented MP4 (ISO/IEC 14496-12): moof + mdat fragments, and the init segment ----------------------
 * hbs_mp4_fragment writes the container around the samples of hbs_annexb_to_lenpref: every fragment is a moof, whose one trun
 * describes its samples, and an mdat that holds them, as DASH / CMAF / fragmented MP4 want them.  The index, the AU numbers and
 * flags of hbs_access_units and the times of hbs_ts_demux / hbs_rtp_unpack are all it reads besides the stream.
 * hbs_mp4_init_host writes the matching init segment on the host.
 *
 * SAMPLES.  AU a is the kept NALs k (d_keep as in hbs_annexb_to_lenpref; NULL: all) with a_k = d_nal_au[k] - d_nal_au[0] == a.
 * Every step d_nal_au[k] - d_nal_au[k-1] is 0 or 1 and a_(n_nals-1) == n_aus - 1 (hbs_rtp_pack's pointer-offset rule: a GOP
 * cut is passed as d_index + first_nal, d_nal_au + first_nal, d_au + first_au).  Of d_au[a] only flags & HBS_AU_IRAP is read.
 * The sample is the records of its kept NALs back to back, exactly as hbs_annexb_to_lenpref makes them: L = length_size bytes
 * of big-endian length, then stream[start, end).  A kept NAL longer than 2^(8 L) - 1 is an error; an AU with nothing kept is a
 * sample of size 0.  B(a) = the record bytes of all AUs below a.
 * TIMES.  dts(a) = d_dts ? d_dts[a] : base_time + a * sample_duration, taken exactly, not wrapped; an exact dts(a) of 2^62 or
 * more is an error at that AU (so is the ~0 "absent" of hbs_ts_demux).  duration(a) = dts(a+1) - dts(a), which must lie in
 * [0, 2^32 - 1]; duration(n_aus - 1) = sample_duration.  cts(a) = (d_pts ? d_pts[a] : dts(a)) - dts(a), which must lie in
 * [-2^31, 2^31 - 1]; a d_pts[a] of 2^62 or more is an error.
 * FRAGMENT CUTS.  s(a) = the largest b <= a with b == 0, or with HBS_MP4_CUT_AT_IRAP set and AU b an IRAP.  AU a begins a
 * fragment iff a == s(a), or max_samples > 0 and (a - s(a)) % max_samples == 0.  Fragment r has first AU f_r and S_r samples.
 * BYTES OF FRAGMENT r (every integer big-endian).  It begins at O_r = B(f_r) + 16 f_r + 96 r and is, with S = S_r:
 *   moof  size 88 + 16 S   'moof'
 *     mfhd  00 00 00 10 'mfhd' 00 00 00 00  sequence(4) = (params->sequence + r) mod 2^32
 *     traf  size 64 + 16 S 'traf'
 *       tfhd  00 00 00 10 'tfhd' 00 02 00 00  track_id(4)                 (default-base-is-moof)
 *       tfdt  00 00 00 14 'tfdt' 01 00 00 00  dts(f_r)(8)
 *       trun  size 20 + 16 S 'trun' 01 00 0F 01  S(4)  data_offset(4) = 96 + 16 S
 *             then per sample: duration(4) size(4) flags(4) cts(4, two's complement)
 *             flags = 0x02000000 for an AU with HBS_AU_IRAP, else 0x01010000
 *   mdat  size 8 + P (4) 'mdat', then the P = B(f_r + S) - B(f_r) sample bytes
 * P > 2^32 - 9 is an error at AU f_r: there is no 64-bit mdat.  So is S > (2^32 - 89) / 16, whose moof size has no 32 bits.
 * Sample a of fragment r lies at O_r + 96 + 16 S_r + B(a) - B(f_r): d_sample_off[a] / d_sample_size[a] (optional, both or
 * neither, n_aus entries each) say so, in exactly the form hbs_lenpref_to_annexb reads.  d_frag[r] (optional, frag_cap
 * entries) is hbs_mp4_frag below.  The output is B(n_aus) + 16 n_aus + 96 R bytes for R fragments:
 * hbs_mp4_fragment_bytes_host(S, P) = 96 + 16 S + P is one fragment's.
 *
 * d_summary: nal_count = fragments R, nal_found = n_nals, rbsp_bytes = B(n_aus), stream_bytes = output bytes, stop_reason = 0,
 * reserved[2] = kept NALs.  error = HBS_E_ARG with reserved[0] = 1 + the lowest offending NAL for an index inconsistent by
 * hbs_filter_annexb's definition, a broken AU-number rule or a record too long for L; HBS_E_ARG with reserved[1] = 1 + the lowest
 * offending AU for a time rule or a fragment-size rule (reported at the fragment's first AU; the fragment sizes are only
 * looked at when no NAL offends).  Either or both may be set; the other counts mean nothing then.  Otherwise HBS_E_CAPACITY when
 * out_cap is below the output or frag_cap < R with a d_frag; the counts are right then.  On any error nothing but the summary
 * is written.  d_out == NULL: plan only, the summary alone is written (the tables are not).  n_nals == 0 with n_aus == 0 is
 * valid: an empty output with no fragment.
 * Refused with HBS_E_ARG at once, before anything is written: a length_size other than 1, 2, 4, unknown flags, track_id 0,
 * base_time of 2^62 or more, n_nals or n_aus above 2^32 - 1, n_nals == 0 with n_aus != 0, out_cap above 2^46 with a d_out, one
 * of the two sample tables without the other, missing or misaligned pointers.
 * Nothing outside [d_out, d_out + output bytes), d_sample_off / d_sample_size[0, n_aus), d_frag[0, R) and the summary is
 * stored; no load touches a 16-byte granule that holds no byte of the stream; the plan reads no stream byte at all (lengths
 * come from the index); no host synchronisation.  Scratch comes from the context's workspace and is sized by n_nals, n_aus and
 * out_cap alone: 16 bytes a NAL and 24 an AU with a d_out (8 an AU without), 64 bytes per 256 NALs, 80 per 256 AUs, and 16
 * bytes per 64 KiB of min(out_cap, stream_bytes + L n_nals + 112 n_aus) -- so pass what the plan gave as out_cap.
 * Alignment: d_stream, d_out, d_au, d_frag, d_summary 16 bytes; d_index, d_dts, d_pts, d_sample_off, d_sample_size 8 bytes;
 * d_nal_au 4 bytes; d_keep any byte.
 * STATED LIMITS: one track; 32-bit mdat and moof sizes; no styp, sidx, prft, emsg, senc or encryption; no edit list (a stream
 * with reordering begins with a positive composition offset).  hbs_mp4_samples, below, reads fragments back.  (The samples can
 * be encrypted in place behind this call -- hbs_cenc_subsamples and hbs_cenc_crypt, below -- but no box says so yet.  The boxes
 * that say so are a call of their own behind this one: hbs_mp4_protect, below.)
 *
 * hbs_mp4_init_host (plain C, no GPU): the init segment for those fragments -- ftyp (iso6, 0, iso6, mp41), then moov with
 * mvhd (rate 0x00010000, volume 0x0100, unity matrix, next_track_ID = track_id + 1), one trak (tkhd flags 3 with
 * width << 16, height << 16; mdia with mdhd, language 0x55C4, hdlr 'vide' "VideoHandler", minf with vmhd flags 1, dinf / dref
 * with one 'url ' of flags 1, stbl with stsd and empty stts, stsc, stsz, stco) and mvex / trex (track_id, description index 1,
 * three zeros).  Every version is 0 and every time and duration 0; mvhd and mdhd carry `timescale`.  The stsd holds one
 * 'hvc1' (HBS_MP4_HEV1: 'hev1') VisualSampleEntry: data_reference_index 1, width, height, 0x00480000 twice, frame_count 1,
 * 32 zero bytes of name, depth 0x0018, 0xFFFF, then the hvcC:
 *   01, the 12 bytes general_profile_space .. general_level_idc of the first SPS among the NALs (bytes [3, 15) of that NAL with
 *   its emulation prevention bytes stripped, the two NAL header bytes counted), F0 00, FC, FC | chroma_format_idc,
 *   F8 | bit_depth_luma - 8, F8 | bit_depth_chroma - 8, 00 00, numTemporalLayers << 3 | temporalIdNested << 2 | length_size - 1
 *   (from stripped byte 2 of that SPS, b: ((b >> 1) & 7) + 1 and b & 1), numOfArrays, and one array each for the types 32, 33,
 *   34 that occur, in that order: array_completeness << 7 | type ('hvc1': 1, 'hev1': 0), the count (2 bytes), then per NAL of
 *   the type, in the given order, its 16-bit length and its bytes.
 * nal[i] / nal_bytes[i], i < n: VPS / SPS / PPS NAL units without start codes.  Returns the bytes the segment takes; it is
 * written to out only when cap suffices.  HBS_E_ARG: a NULL pointer, unknown flags, n of 0 or above 65535, track_id 0 or
 * 2^32 - 1, timescale 0, width or height outside 1..65535, a length_size other than 1, 2, 4, chroma_format_idc outside 0..3, a
 * bit depth outside 8..15 (the hvcC has three bits for each), a NAL shorter than 2 bytes or longer than 65535, a NAL type
 * outside 32..34, no SPS, an SPS with fewer than 15 bytes once stripped.  Every length is bounded before it is used; no byte
 * outside the NALs is read.
 */
typedef struct hbs_mp4_params {   /* HOST memory, 32 bytes */
    int32_t  length_size;      /* 1, 2 or 4: as hbs_annexb_to_lenpref */
    uint32_t flags;            /* HBS_MP4_* */
    uint32_t track_id;         /* 1 .. 2^32 - 1 */
    uint32_t sequence;         /* mfhd sequence_number of the call's first fragment; fragment r carries (sequence + r) mod 2^32 */
    uint32_t max_samples;      /* 0: no limit; else no fragment holds more samples */
    uint32_t sample_duration;  /* duration of the call's last AU, and of every AU when d_dts == NULL */
    uint64_t base_time;        /* with d_dts == NULL: dts(a) = base_time + a * sample_duration */
} hbs_mp4_params;
#define HBS_MP4_CUT_AT_IRAP 1u  /* a fragment begins at every AU with HBS_AU_IRAP */

typedef struct hbs_mp4_frag {     /* 48 bytes */
    uint64_t out_off, out_bytes;  /* the fragment (moof + mdat) in the output */
    uint64_t first_au;            /* its first sample, numbered within the call */
    uint64_t decode_time;         /* tfdt baseMediaDecodeTime */
    uint32_t samples, sequence, flags /* HBS_AU_IRAP when its first sample is one */, reserved;
} hbs_mp4_frag;

struct hbs_access_unit;            /* hbs_access_units' record, below */
int hbs_mp4_fragment(hbs_ctx* ctx, const uint8_t* d_stream, uint64_t stream_bytes,
                     const hbs_nal_entry* d_index, uint64_t n_nals, const uint8_t* d_keep /* nullable */,
                     const uint32_t* d_nal_au, const struct hbs_access_unit* d_au, uint64_t n_aus,
                     const uint64_t* d_dts /* nullable */, const uint64_t* d_pts /* nullable */,
                     const hbs_mp4_params* params,
                     uint8_t* d_out, uint64_t out_cap,
                     uint64_t* d_sample_off, uint64_t* d_sample_size /* optional, both or neither, n_aus */,
                     hbs_mp4_frag* d_frag /* optional */, uint64_t frag_cap,
                     hbs_summary* d_summary);
uint64_t hbs_mp4_fragment_bytes_host(uint64_t samples, uint64_t sample_bytes);   /* 96 + 16 S + bytes */

typedef struct hbs_mp4_init_params {  /* 32 bytes */
    uint32_t track_id, timescale, width, height;    /* width, height: 1..65535 */
    int32_t  length_size;                            /* 1, 2, 4 */
    int32_t  chroma_format_idc, bit_depth_luma, bit_depth_chroma;   /* 0..3, 8..15, 8..15 */
} hbs_mp4_init_params;
#define HBS_MP4_HEV1 1   /* sample entry 'hev1' (sets may also be in band), array_completeness 0; default 'hvc1', 1 */
int64_t hbs_mp4_init_host(const hbs_mp4_init_params* p, int flags,
                          const uint8_t* const* nal, const uint64_t* nal_bytes, uint64_t n /* VPS / SPS / PPS NALs, no start codes */,
                          uint8_t* out, uint64_t cap);   /* bytes needed; written only when cap suffices; HBS_E_ARG */

/*
 * ---- fragmented MP4 -> sample table: moof, traf, tfhd, tfdt, trun read on the device; the init segment on the host -------
 * hbs_mp4_samples turns the moof boxes of CMAF / DASH / fMP4 segments that lie in device memory into what
 * hbs_lenpref_to_annexb reads -- per sample its offset and size -- and into decode time, presentation time and flags, with
 * one hbs_mp4_frag a moof.  It reads what other muxers write: optional fields, three levels of defaults, 64-bit box sizes,
 * several truns, data offsets that continue.  hbs_mp4_init_read_host reads the init segment on the host: length_size for
 * hbs_lenpref_to_annexb, the trex defaults for hbs_mp4_read_params.  Every integer in a box is big-endian.
 *
 * SEGMENTS.  Segment i is d_in[off_i, off_i + size_i): off_i and size_i are the first two uint64_t of the record at
 * d_seg + i * seg_stride, seg_stride a multiple of 8 and at least 16.  A stride of 16 is a plain table; a stride of 48 takes
 * d_frag of hbs_mp4_fragment as it is (out_off and out_bytes are its first two fields).  d_seg == NULL: one segment, the whole
 * buffer; n_segs is ignored.  A segment is a chain of top-level boxes that tiles it exactly.  A BOX at p in a container that
 * ends at e is size(4) type(4); size == 1: a 64-bit largesize follows the type and is the size, which must be 16 or more;
 * size == 0: the box runs to e; any other size below 8 is an error; so are fewer than 8 bytes (16 with a largesize) between p
 * and e, and a size larger than e - p.  The next box is at p + size; the chain ends when p == e.  Any type other than 'moof'
 * is stepped over (styp, sidx, prft, emsg, free, mdat, ftyp, moov ...).  A box that breaks a rule is a CHAIN ERROR at that
 * segment; so is a segment that leaves the buffer (off_i + size_i > in_bytes, or the sum wraps).
 * One lane walks one segment's chain, twice (to count the moofs, and to place them once their numbers are known), as
 * hbs_lenpref_to_annexb does for a sample's records.  So a buffer of very many fragments passed as ONE segment is walked by one
 * lane, at the latency of one dependent load a box: pass a segment table (a record a fragment, or a few) to avoid that.
 *
 * INSIDE A MOOF.  The children of moof and traf are chained by the same rule, the container's end for e; unknown children are
 * stepped over at every level (senc, saiz, saio, sbgp, sgpd, uuid ...).  A child that breaks the rule is a MOOF ERROR, as is
 * everything called an error below.  Of several mfhd, tfhd or tfdt in one container the first is read.
 *   mfhd  payload (behind the box header) version/flags(4) sequence(4): the version must be 0 and the payload 8 bytes or more.
 *         A moof without an mfhd is an error.
 *   traf  the one read is the first whose tfhd carries params->track_id; with track_id == 0 the first.  Every traf in front of
 *         it must have a well-formed tfhd.  Later trafs, of the same track too, are not looked at (a stated limit).  A moof
 *         without such a traf is a fragment of 0 samples.
 *   tfhd  version/flags(4) track_id(4), then by flag: 0x000001 base_data_offset(8), 0x000002 sample_description_index(4,
 *         skipped), 0x000008 default duration(4), 0x000010 default size(4), 0x000020 default flags(4); a payload shorter than
 *         those fields is an error.  0x020000 is default-base-is-moof; 0x010000 (duration-is-empty) and the version are ignored.
 *         BASE: with 0x000001, off_i + base_data_offset (the offset within the segment's file); otherwise the moof's first
 *         byte -- except for a traf that is not its moof's first and sets neither 0x000001 nor 0x020000: the standard's "end of
 *         the previous traf's data" is not supported, an error.
 *   tfdt  version/flags(4), then the time: version 0 32 bits, version 1 64 bits; any other version, a shorter payload or no
 *         tfdt in the traf that is read is an error (a stated limit: CMAF and DASH require the box).
 *   trun  version/flags(4) count(4), then by flag 0x001 data_offset(4, signed), 0x004 first_sample_flags(4), then count
 *         entries of, by flag and in this order, 0x100 duration(4), 0x200 size(4), 0x400 flags(4), 0x800 composition
 *         offset(4: version 0 unsigned, version 1 signed): 4 x popcount(flags & 0xF00) bytes an entry.  8 + 4 [0x001] +
 *         4 [0x004] + count x entry must not exceed the payload; a version above 1 is an error.  Any number of truns, in
 *         order.  DATA BEGIN: with 0x001, base + data_offset; without, where the previous trun of the traf ended (a trun of
 *         count 0 with 0x001 ends at its data begin); the traf's first trun without 0x001 begins at base.
 *
 * SAMPLES are numbered through the call in segment, moof, trun and entry order.  size = the entry's, else the tfhd's, else
 * params->trex_size; duration the same way.  flags = the entry's, else first_sample_flags for entry 0 of a trun with 0x004,
 * else the tfhd's, else trex_flags.  offset = the trun's data begin + the sizes of the trun's earlier entries.  dts = the tfdt
 * time + the durations of all earlier samples of the moof, across its truns; pts = dts + composition offset; all exact, not
 * wrapped.  A SAMPLE ERROR: dts of 2^62 or more, pts outside [0, 2^62), offset + size > in_bytes, a negative data begin.
 * d_sample_off / d_sample_size are exactly what hbs_lenpref_to_annexb reads, d_dts / d_pts what hbs_mp4_fragment, hbs_ts_mux and
 * hbs_rtp_pack read.  d_sample_flags is the raw 32-bit word: a sync sample is one with bit 0x00010000
 * (sample_is_non_sync_sample) clear.
 *
 * FRAGMENT TABLE.  d_frag[m] for moof m (numbered through the call): out_off = its offset in d_in; out_bytes = the distance
 * to the next moof of the same segment, or to the segment's end; first_au = its first sample's number; decode_time = the tfdt
 * time; samples; sequence = the mfhd's; flags = HBS_AU_IRAP iff it has a sample and its first sample is a sync sample;
 * reserved = 0.  On the output of hbs_mp4_fragment, one segment a fragment or all in one, this is that call's d_frag field
 * for field.
 *
 * d_summary: nal_count = samples N, nal_found = moofs M, rbsp_bytes = the sum of the sample sizes, stream_bytes = in_bytes,
 * stop_reason = 0.  The stages are looked at in this order and the first that fails ends the call:
 *   a chain error          error = HBS_E_ARG, reserved[0] = 1 + the lowest such segment; no count means anything
 *   M > moof_cap           error = HBS_E_CAPACITY; nal_found = M is right, the moofs were not read: nal_count = rbsp_bytes = 0
 *   a moof error           error = HBS_E_ARG, reserved[1] = 1 + the lowest such moof; M is right, nal_count = rbsp_bytes = 0
 *   N > sample_cap         (with outputs) error = HBS_E_CAPACITY; M and N are right, the samples were not read: rbsp_bytes = 0
 *   a sample error         error = HBS_E_ARG, reserved[2] = 1 + the lowest such sample; M and N are right, rbsp_bytes = 0
 * reserved words not named are 0.  On any error nothing but the summary is written.  d_sample_off == NULL: plan only, the
 * summary alone is written and sample_cap sizes nothing -- moof_cap still sizes the moofs' scratch, and each moof's lane goes
 * through its entries itself: one lane a moof, a step an entry that has bytes (so a moof's plan is bounded by its size, and a
 * moof of one very large trun is planned by one lane, at the cost per entry that profiles/r19/mp4rd_time.txt records); a trun
 * whose entries have no bytes, whose count nothing in the box bounds, is settled in closed form whatever its count.  n_segs == 0 with a d_seg is valid and gives nothing; so is an empty buffer as one segment.
 * Refused with HBS_E_ARG at once: params->flags != 0 (none is defined), non-zero reserved words, a seg_stride below 16 or not
 * a multiple of 8 (with a d_seg), n_segs above 2^32 - 1, in_bytes above 2^62, one sample table without the other, d_dts, d_pts,
 * d_sample_flags or d_frag without the sample tables, moof_cap above 2^32 - 1, sample_cap above 2^32 - 1 with outputs, missing
 * or misaligned pointers.
 * Nothing outside d_sample_off / d_sample_size / d_dts / d_pts / d_sample_flags[0, N), d_frag[0, M) and the summary is stored;
 * no load touches a 16-byte granule that holds no byte of d_in[0, in_bytes); no mdat payload byte is read (only box headers
 * along the chains and the boxes named above); no host synchronisation.  Scratch comes from the context's workspace and is
 * sized by n_segs, moof_cap and sample_cap alone: 8 bytes a segment, 96 bytes a moof of moof_cap, with outputs 68 bytes a
 * sample of sample_cap, and 64, 128 and 128 bytes per 256 of each.  The grids are sized the same way -- so pass what the plan
 * gave, not "plenty".
 * Alignment: d_in, d_frag, d_summary 16 bytes; d_seg and the four 64-bit tables 8 bytes; d_sample_flags 4 bytes.
 * STATED LIMITS: one track a call; a missing tfdt is an error; the "end of the previous traf's data" base is not supported;
 * no encryption (senc, saiz, saio are stepped over; the samples stay as they are); no sidx-driven access (pass the segments);
 * a file without fragments is read by hbs_mp4_stbl_samples, below; one lane walks a segment's chain.  (hbs_cenc_crypt, below,
 * decrypts samples in place from the tables this call writes, given their subsample table and IVs from elsewhere.)
 * (That elsewhere can be the fragments themselves: hbs_mp4_senc_samples, below, reads both from the senc boxes of the fragments
 * d_frag names, and hbs_mp4_init_unprotect_host turns an 'encv' init segment into one hbs_mp4_init_read_host accepts.)
 *
 * hbs_mp4_init_read_host (plain C, no GPU): the counterpart of hbs_mp4_init_host.  It walks seg[0, n) by the box rule above:
 * moov; its trak boxes in order -- tkhd (version 0 or 1: track_id, width and height, the integer parts), mdia / mdhd (version
 * 0 or 1: timescale), mdia / minf / stbl / stsd, whose first 'hvc1' or 'hev1' entry that holds an hvcC is the one read --
 * and mvex / trex of that track (its three defaults).  The stsd's entries are taken one at a time, entry_count of them at
 * the most, each held to the box rule when it is reached, and nothing behind the entry that is chosen is looked at.
 * track_id 0: the first trak with such an entry.  From the hvcC:
 * length_size = (byte 21 & 3) + 1, and for every array in order every NAL's offset and size within seg.  Returns the number
 * of those NALs; nal_off / nal_bytes are written for the first `cap` of them (so call with cap 0 first, or with room for
 * out->n_nals).  HBS_E_ARG: a NULL seg or out, anything malformed or missing (a box that breaks the size rule, no moov, no such
 * track or one without an hvcC, a tkhd / mdhd version above 1 or a payload too short for its fields, an hvcC whose version
 * byte is not 1 or whose arrays leave it, no trex for the track).  Every length is bounded before it is used; no byte at or
 * behind seg + n is read.  On the output of hbs_mp4_init_host it returns what went in.
 */
typedef struct hbs_mp4_read_params {   /* HOST memory, 32 bytes */
    uint32_t flags;                    /* none defined yet: must be 0 */
    uint32_t track_id;                 /* the track whose traf is read; 0: the first traf of every moof */
    uint32_t trex_duration, trex_size, trex_flags;   /* defaults of the init segment's trex */
    uint32_t reserved[3];              /* 0 */
} hbs_mp4_read_params;

int hbs_mp4_samples(hbs_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes,
                    const void* d_seg /* nullable */, uint64_t seg_stride, uint64_t n_segs,
                    const hbs_mp4_read_params* params,
                    uint64_t moof_cap, uint64_t sample_cap,
                    uint64_t* d_sample_off, uint64_t* d_sample_size,   /* both or neither; NULL: plan only */
                    uint64_t* d_dts, uint64_t* d_pts,                  /* optional, each on its own */
                    uint32_t* d_sample_flags,                          /* optional */
                    hbs_mp4_frag* d_frag /* optional, moof_cap entries */,
                    hbs_summary* d_summary);

typedef struct hbs_mp4_track {      /* 64 bytes */
    uint32_t track_id, timescale, width, height;
    int32_t  length_size;           /* lengthSizeMinusOne + 1 */
    uint32_t entry;                 /* fourcc: 'hvc1' or 'hev1' */
    uint32_t trex_duration, trex_size, trex_flags;
    uint32_t n_nals;                /* parameter-set NALs in the hvcC, all arrays */
    uint64_t hvcc_off, hvcc_bytes;  /* the hvcC payload within the segment */
    uint32_t reserved[2];
} hbs_mp4_track;
int64_t hbs_mp4_init_read_host(const uint8_t* seg, uint64_t n, uint32_t track_id /* 0: the first video track with an hvcC */,
                               hbs_mp4_track* out, uint64_t* nal_off, uint64_t* nal_bytes, uint64_t cap);

/*
 * ---- progressive MP4 -> sample table: stsz, stco / co64, stsc, stts, ctts, stss read on the device; the boxes found on the host
 * A plain .mp4 / .mov is one moov whose stbl describes every sample, and one mdat.  hbs_mp4_stbl_find_host finds the six table
 * boxes of one track; hbs_mp4_stbl_samples reads them from device memory and writes what hbs_mp4_samples writes for
 * fragments: per sample its offset and size (what hbs_lenpref_to_annexb reads), decode time, presentation time and flags.
 * Every integer in a box is big-endian; the tables lie at any byte alignment.
 *
 * hbs_mp4_stbl_find_host (plain C, no GPU) walks seg[0, n) by the box rule stated above hbs_mp4_samples and finds the moov and
 * the trak exactly as hbs_mp4_init_read_host does (one walk serves both; track_id 0: the first track with an hvcC), then the
 * children of its mdia / minf / stbl.  Of several boxes of one type the first is used, of stco and co64 whichever comes first.
 * Every `off` is the payload's offset within seg (behind the box header) plus `base`: a caller who passes only the moov cut
 * from file position P passes base = P and gets file offsets.  file_bytes is left 0.  HBS_E_ARG: a NULL seg or out, n above
 * 2^62, a malformed chain, no such track, no stsz, stsc or stts, neither stco nor co64 (a stz2 without a stsz is such a file:
 * compact sample sizes are a stated limit), one of the table boxes with an empty payload.  No byte at or behind seg + n is
 * read.  The edit list (elst) is not applied: times are the media's (a stated limit).
 * hbs_mp4_track_read_host is hbs_mp4_init_read_host for such a file: the same walk, the same record and parameter-set NALs
 * (length_size for hbs_lenpref_to_annexb, the sets for hbs_au_insert), but no mvex is asked for -- a progressive file has
 * none -- and the three trex fields of the record are 0.
 *
 * hbs_mp4_stbl_samples reads the boxes from d_in at the offsets in `tables`.  The rules, every payload beginning with
 * version/flags(4):
 *   stsz  sample_size(4) count N(4), then N sizes(4) iff sample_size == 0.  With sample_size != 0 nothing in the box bounds N.
 *   stco  count C(4), then C chunk offsets(4);  co64 (HBS_MP4_STBL_CO64): offsets(8).
 *   stsc  count E(4), then E entries first_chunk(4) samples_per_chunk(4) description index(4, ignored: a stated limit).
 *         first_chunk is 1 in entry 0, strictly increasing, and at most C.  Entry e covers the chunks up to the next entry's
 *         first_chunk, the last entry up to C.  samples_per_chunk 0 is valid: those chunks hold no sample.  The chunks must
 *         hold N samples or more between them; surplus chunks and surplus room in the last chunk used are ignored.
 *   stts  count(4), then entries sample_count(4) delta(4).  The counts must sum to N or more; surplus is ignored; entries of
 *         count 0 are valid.
 *   ctts  (optional) count(4), then entries sample_count(4) offset(4): unsigned at version 0, signed at version 1; a version
 *         above 1 is an error.  Counts that sum to less than N leave the remaining samples at offset 0.
 *   stss  (optional) count(4), then 1-based sample numbers(4), strictly increasing, none 0; numbers above N are ignored.
 *         Absent: every sample is a sync sample.  Present and empty: none is.
 * The versions of stsz, stco, co64, stsc, stts and stss must be 0; a payload shorter than its fixed part plus count x entry is
 * an error.
 * SAMPLE s, in table order: size from stsz; off = its chunk's offset + the sizes of the earlier samples of that chunk; dts =
 * the sum of the earlier samples' deltas; pts = dts + composition offset; flags = 0 for a sync sample, 0x00010000 for any other
 * (the bit hbs_mp4_samples documents).  All sums are exact 64-bit quantities and none wraps into a success: counts and
 * samples_per_chunk of 2^32 - 1 are legal inputs to the checks.
 *
 * The stages are looked at in this order and the first that fails ends the call; on any error only the summary is written:
 *   a table error     error = HBS_E_ARG, reserved[0] = 1 + the first broken box in the order stsz, stco, stsc, stts, ctts, stss
 *                     (the coverage rules count at stsc and stts); no count means anything
 *   N > sample_cap    (with outputs) error = HBS_E_CAPACITY; nal_count = N and nal_found = C are right, rbsp_bytes = 0
 *   a sample error    (looked for only with outputs) error = HBS_E_ARG, reserved[2] = 1 + the lowest such sample: off + size
 *                     above file_bytes (in_bytes when that is 0), an offset sum that wraps, dts of 2^62 or more, pts outside
 *                     [0, 2^62); N and C are right, rbsp_bytes = 0
 * d_summary: nal_count = N, nal_found = C, rbsp_bytes = the sum of the sizes, stream_bytes = in_bytes, stop_reason = 0.
 * d_sample_off == NULL: plan only -- the table errors are looked for and the summary is written; sample_cap sizes nothing.
 * WORK.  Grids and scratch are sized by the payload byte counts in `tables` and by sample_cap (a table cannot have more entries
 * than its bytes allow), never by a count read from a box: a stsz of constant size or a stts of one entry that claims
 * 2^32 - 1 samples costs a plan no more than an honest one.  With outputs the work is bounded by sample_cap plus the entries.
 * Scratch: 64 bytes per 256 entries of the longest of stsc / stts / ctts / stss; plan only 64 bytes per 256 sizes of a stsz;
 * with outputs 8 bytes an entry of stsc and ctts, 16 an entry of stts, and 128 bytes per 256 samples of sample_cap.
 * Refused with HBS_E_ARG at once: unknown flags or non-zero reserved words; a required box (stsz, stco, stsc, stts) with
 * bytes == 0, or a box that leaves d_in[0, in_bytes); in_bytes or file_bytes above 2^62; sample_cap above 2^32 - 1 with
 * outputs; one sample table without the other, or d_dts, d_pts or d_sample_flags without the sample tables; missing or
 * misaligned pointers.  Alignment: d_in and d_summary 16 bytes, the four 64-bit tables 8, d_sample_flags 4.
 * Nothing outside d_sample_off / d_sample_size / d_dts / d_pts / d_sample_flags[0, N) and the summary is stored; no load
 * touches a 16-byte granule that holds no byte of d_in[0, in_bytes); no mdat byte is read; no host synchronisation and no
 * allocation once the scratch has its size.
 * STATED LIMITS: one track a call; no stz2 (compact sample sizes); the edit list is not applied; the sample description index
 * is ignored (one sample entry); no encryption (the samples stay as they are; hbs_cenc_crypt, below, works on the tables
 * this call writes, given the subsample table and IVs from elsewhere).
 */
#define HBS_MP4_STBL_CO64 1u           /* hbs_mp4_stbl.flags: .stco refers to a co64 (64-bit entries) */
typedef struct hbs_mp4_box_ref { uint64_t off, bytes; } hbs_mp4_box_ref;  /* the payload behind the box header; bytes == 0: no such box */
typedef struct hbs_mp4_stbl {        /* HOST memory, 128 bytes */
    hbs_mp4_box_ref stsz, stco, stsc, stts, ctts, stss;   /* stco: the stco or the co64 */
    uint32_t flags;                  /* HBS_MP4_STBL_CO64: .stco refers to a co64 (64-bit entries) */
    uint32_t reserved0;              /* 0 */
    uint64_t file_bytes;             /* what sample offsets are checked against; 0: in_bytes of the device call */
    uint64_t reserved[2];            /* 0 */
} hbs_mp4_stbl;
int hbs_mp4_stbl_find_host(const uint8_t* seg, uint64_t n, uint64_t base, uint32_t track_id, hbs_mp4_stbl* out);
int64_t hbs_mp4_track_read_host(const uint8_t* seg, uint64_t n, uint32_t track_id /* 0: the first video track with an hvcC */,
                                hbs_mp4_track* out, uint64_t* nal_off, uint64_t* nal_bytes, uint64_t cap);

int hbs_mp4_stbl_samples(hbs_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes,
                         const hbs_mp4_stbl* tables,          /* host memory */
                         uint64_t sample_cap,
                         uint64_t* d_sample_off, uint64_t* d_sample_size,   /* both or neither; NULL: plan only */
                         uint64_t* d_dts, uint64_t* d_pts,                  /* optional, each on its own */
                         uint32_t* d_sample_flags,                          /* optional */
                         hbs_summary* d_summary);

/*
 * ---- sample table -> progressive MP4: stts, ctts, stss, stsc, stsz, stco / co64 written on the device; the moov around them on the host
 * The counterpart of hbs_mp4_stbl_samples.  hbs_mp4_stbl_write takes the per-sample tables that hbs_annexb_to_lenpref,
 * hbs_mp4_fragment, hbs_mp4_samples and hbs_mp4_stbl_samples write -- offset and size, optionally decode time, presentation
 * time and flags -- and writes the children of a stbl behind its stsd; hbs_mp4_moov_host writes ftyp and the moov up to and
 * including that stsd.  With the caller's 8 bytes of mdat header and the sample bytes, which already lie on the device, that is
 * a whole .mp4.  No sample byte (mdat) is read.
 *
 * OUTPUT.  d_out receives whole boxes in this order: stts, ctts (iff d_pts), stss (iff d_sample_flags), stsc, stsz, then stco or,
 * with HBS_MP4_STBL_CO64, co64.  Each is size(4) type(4) version/flags(4) = 0 (ctts: see below), then the payload exactly as
 * the section above specifies it for the reader.  Every integer is big-endian, every box size a multiple of 4; the T bytes of
 * the six boxes are written with 32-bit stores and no byte outside [d_out, d_out + T) is touched.
 * THE RULES, with N = n_samples, o(k) = d_sample_off[k] + data_offset and z(k) = d_sample_size[k]:
 *   CHUNKS  Sample k is contiguous iff k > 0 and d_sample_off[k] == d_sample_off[k-1] + z(k-1), taken exactly.  s(k) is the
 *           largest j <= k that is not contiguous.  Sample k begins a chunk iff k == s(k), or max_chunk_samples > 0 and
 *           (k - s(k)) % max_chunk_samples == 0 (the form of hbs_mp4_fragment's cut rule).  There are C chunks; chunk c has the
 *           first sample f_c and L_c samples.
 *   stco    count C, then o(f_c) in 32 bits; co64: in 64 bits.
 *   stsc    an entry (c + 1, L_c, 1) for every chunk c with c == 0 or L_c != L_(c-1); N == 0: no entry.
 *   stsz    if N > 0, every z(k) equals z(0) and z(0) != 0: sample_size = z(0), count N, no table.  Otherwise sample_size = 0,
 *           count N, then the N sizes.
 *   stts    dts(k) = d_dts ? d_dts[k] : base_time + k * sample_duration, exactly.  delta(k) = dts(k+1) - dts(k); delta(N-1),
 *           and every delta when d_dts == NULL, is sample_duration.  The entries are run-length: an entry begins at k == 0 and
 *           wherever delta(k) != delta(k-1).  d_dts == NULL: one entry (N, sample_duration), none for N == 0.
 *   ctts    written iff d_pts != NULL, even when every offset is 0.  cts(k) = d_pts[k] - dts(k), run-length in the same way;
 *           version 1 (signed offsets) iff some cts(k) < 0, else version 0.
 *   stss    written iff d_sample_flags != NULL, even when empty: the 1-based numbers of the samples with
 *           (d_sample_flags[k] & 0x00010000) == 0, ascending.
 * A SAMPLE ERROR, all taken exactly in 64 bits: z(k) above 2^32 - 1; an o(k) that wraps, or o(k) + z(k) at or above 2^62;
 * without HBS_MP4_STBL_CO64 a chunk's o(f_c) above 2^32 - 1, reported at f_c; dts(k) of 2^62 or more; a delta(k) outside
 * [0, 2^32 - 1], reported at k; d_pts[k] of 2^62 or more; cts(k) outside [-2^31, 2^31 - 1].
 * A BOX SIZE ERROR: a box whose size would pass 2^32 - 1 (an stts, ctts or stsc of 2^29 entries or so and more, a co64 or an
 * stsz or stss of near 2^32).
 *
 * d_summary: nal_count = N, nal_found = C, rbsp_bytes = the sum of the z(k), stream_bytes = T, stop_reason = 0, reserved[1] =
 * the sum of all deltas (the media duration for hbs_mp4_moov_host).  The stages are looked at in this order and the first that
 * fails ends the call:
 *   a sample error     error = HBS_E_ARG, reserved[2] = 1 + the lowest such sample; only nal_count means anything
 *   a box size error   error = HBS_E_ARG, reserved[0] = 1 + the box, numbered in the output's order (stts 0 .. stco / co64 5);
 *                      only nal_count means anything
 *   out_cap < T        (with a d_out) error = HBS_E_CAPACITY; the counts, T and the duration are right
 * On any error nothing but the summary is written.  d_out == NULL: plan only -- the same checks run, the summary and d_tables
 * are written.  T does not depend on data_offset, because stco or co64 is the caller's flag, not chosen from the offsets: so a
 * plan gives the T that the real call will write.
 * d_tables (optional, DEVICE memory) is the hbs_mp4_stbl that hbs_mp4_stbl_find_host would fill for these boxes with a base
 * that makes d_out offset 0: payload offsets behind the 8-byte box headers, bytes == 0 for an absent ctts / stss, flags = the
 * CO64 bit, file_bytes = 0, reserved words 0.  Copied to the host it is the `tables` argument of hbs_mp4_stbl_samples.
 * Refused with HBS_E_ARG at once: unknown flags or a non-zero reserved0; n_samples above 2^32 - 1; base_time or data_offset of
 * 2^62 or more; out_cap above 2^46 with a d_out; a missing d_summary or params, missing sample tables with n_samples > 0;
 * misaligned pointers.  Alignment: the four 64-bit tables 8 bytes, d_sample_flags 4, d_out, d_tables and d_summary 16.
 * n_samples == 0 is valid: four boxes of count 0 (68 bytes), plus a ctts / stss of count 0 if asked for.
 * hbs_mp4_stbl_write_bytes_host: an upper bound of T -- an entry a sample in every box -- for a caller who does not plan; 0 for
 * n_samples above 2^32 - 1.
 * GUARANTEES: no host synchronisation; no allocation once the scratch has its size; the scratch comes from the context's
 * workspace and is sized by n_samples alone (24 bytes a sample, 200 bytes per 256 samples, 256 bytes); every grid is sized by
 * n_samples, never by a count computed on the device; no sample byte is read.
 *
 * hbs_mp4_moov_host (plain C, no GPU) writes ftyp and the moov up to and including the stsd: everything as hbs_mp4_init_host
 * specifies it, except that there is no mvex, the stbl holds the stsd alone (no empty tables), mvhd, tkhd and mdhd carry
 * `duration`, and the sizes of moov, trak, mdia, minf and stbl already count tables_bytes more than is written.  The stbl is the
 * last child all the way up, so this prefix followed by the T bytes of hbs_mp4_stbl_write (tables_bytes = T, duration =
 * reserved[1] of its summary) is a complete moov.  Returns the bytes of the prefix; it is written only when cap suffices.
 * HBS_E_ARG: everything hbs_mp4_init_host refuses; a duration above 2^32 - 1 (the boxes are version 0: a stated limit); a
 * tables_bytes that is not a multiple of 4; a tables_bytes that takes the moov past 2^32 - 1.
 * THE TWO FILE LAYOUTS.  The mdat header is the caller's 8 bytes: size(4) = 8 + the sample bytes, 'mdat'; the size has 32
 * bits, so the samples of one file stay below 2^32 - 8 bytes (there is no 64-bit mdat: a stated limit).
 *   ftyp + mdat + moov   one call: the prefix has F bytes of ftyp (its first box), data_offset = F + 8; the file is ftyp, the
 *                        mdat header, the samples, the prefix behind its ftyp, the T bytes.
 *   ftyp + moov + mdat   plan first (d_out == NULL) and read T from the summary; the prefix has P bytes; then the real call
 *                        with data_offset = P + T + 8; the file is the prefix, the T bytes, the mdat header, the samples.
 * STATED LIMITS: one track; no edit list (a stream with reordering begins with a positive composition offset); no stz2; no
 * sdtp; one sample entry (every stsc entry names description 1); no encryption (hbs_cenc_crypt, below, encrypts the samples
 * in place, but no box written here says so).
 */
typedef struct hbs_mp4_stbl_write_params {   /* HOST memory, 32 bytes */
    uint32_t flags;              /* HBS_MP4_STBL_CO64: write a co64; otherwise a stco */
    uint32_t max_chunk_samples;  /* 0: chunks are cut by contiguity alone */
    uint32_t sample_duration;    /* delta of the last sample, and of every sample when d_dts == NULL */
    uint32_t reserved0;          /* 0 */
    uint64_t base_time;          /* with d_dts == NULL: dts(k) = base_time + k * sample_duration */
    uint64_t data_offset;        /* added to every d_sample_off[k]: where the sample bytes will lie in the file */
} hbs_mp4_stbl_write_params;

int hbs_mp4_stbl_write(hbs_ctx* ctx,
                       const uint64_t* d_sample_off, const uint64_t* d_sample_size, uint64_t n_samples,
                       const uint64_t* d_dts /* nullable */, const uint64_t* d_pts /* nullable */,
                       const uint32_t* d_sample_flags /* nullable */,
                       const hbs_mp4_stbl_write_params* params,
                       uint8_t* d_out /* NULL: plan only */, uint64_t out_cap,
                       hbs_mp4_stbl* d_tables /* optional, DEVICE memory, 128 bytes, 16-aligned */,
                       hbs_summary* d_summary);
uint64_t hbs_mp4_stbl_write_bytes_host(uint64_t n_samples, int with_ctts, int with_stss, uint32_t flags);  /* upper bound */
int64_t hbs_mp4_moov_host(const hbs_mp4_init_params* p, int flags,
                          const uint8_t* const* nal, const uint64_t* nal_bytes, uint64_t n,
                          uint64_t duration, uint64_t tables_bytes,
                          uint8_t* out, uint64_t cap);   /* bytes needed; written only when cap suffices; HBS_E_ARG */

/*
 * ---- MPEG transport stream (ISO/IEC 13818-1) -> Annex-B elementary stream, PES times ----------------------------------
 * hbs_ts_demux takes the packets of one PID out of a transport stream in device memory and writes their elementary-stream
 * bytes back to back: the Annex-B stream hbs_index_extract / hbs_index_parse_compact take.  With it comes a table of the
 * PES packets begun, each with its PTS / DTS and the output offset of its first byte; a muxer that puts one access unit
 * into one PES packet makes that offset hbs_access_unit.unit_begin, which is how a time finds its sample.
 *
 * THE PACKET RULE.  B = packet_bytes is 188, 192 (M2TS: a 4-byte time prefix in front) or 204 (16 Reed-Solomon bytes
 * behind); anything else is HBS_E_ARG at once.  Packet p is d_ts[p B, (p + 1) B); its 188 transport bytes b[] begin at
 * h = 4 when B == 192, else at h = 0; the other bytes of the packet are ignored.  In this order:
 *   sync fault    b[0] != 0x47: a FAULT, whatever the PID.
 *   fields        tei = b[1] >> 7, pusi = (b[1] >> 6) & 1, pid = (b[1] & 0x1F) << 8 | b[2], tsc = b[3] >> 6,
 *                 afc = (b[3] >> 4) & 3, cc = b[3] & 15.
 *   other PID     pid != the wanted one: the packet plays no further part (HBS_TS_OTHER).
 *   skipped       tei set or tsc != 0: HBS_TS_SKIPPED -- counted, not copied, nothing else of it is looked at.
 *   adaptation    off = 4.  With afc & 2: afl = b[4]; afl > 183 is a FAULT; off = 5 + afl; with afl >= 1,
 *                 discontinuity_indicator = b[5] >> 7 and random_access_indicator = (b[5] >> 6) & 1 (else both 0).
 *   payload       (afc & 1) == 0 or off == 188: HBS_TS_NO_PAYLOAD -- neither copied nor counted as skipped, pusi ignored.
 *                 Else the payload is b[off, 188), len = 188 - off.
 *   PES start     with pusi the payload begins a PES packet q[] = b[off ...]: len >= 9, q[0..2] == 00 00 01,
 *                 (q[6] & 0xC0) == 0x80, f = q[7] >> 6 is not 1, H = 9 + q[8] <= len, q[8] >= 5 when f == 2 and >= 10 when
 *                 f == 3 must all hold, else FAULT.  HBS_TS_PES_START; its ES bytes are q[H, len) (there may be none).
 *                 Without pusi the ES bytes are the whole payload (HBS_TS_PAYLOAD).
 *   times         PTS from q[9..13] (f >= 2), DTS from q[14..18] (f == 3), each as
 *                 ((x0 >> 1) & 7) << 30 | x1 << 22 | (x2 >> 1) << 15 | x3 << 7 | x4 >> 1.  Marker bits are not checked,
 *                 PES_packet_length is not used.
 * STATED LIMIT: a PES header that does not end inside the packet it begins in is a fault (H > len); it is not followed
 * into the next packet.
 *
 * THE CALL.  ts_bytes must be a multiple of packet_bytes and hold at most 2^32 - 1 packets, pid is 0..8191; anything else
 * is refused with HBS_E_ARG at once, before anything is written.  ts_bytes == 0 is valid.
 * Let C be the packets of the PID with HBS_TS_PAYLOAD or HBS_TS_PES_START that lie at or behind the first HBS_TS_PES_START
 * packet of the PID, in order.  Every packet of the PID in front of that first PES start (all of them when there is none)
 * counts as skipped, whatever its class.  The output is the ES bytes of C, back to back.  d_pes (optional) receives one
 * record per PES start in C, in order.  d_out == NULL: plan only -- the summary alone is written, no capacity is looked at.
 *   d_summary   nal_count = PES packets begun; nal_found = packets of the PID, whatever their class; stream_bytes = output
 *               bytes; rbsp_bytes = 0; stop_reason = 0;
 *               reserved[1] = continuity breaks: members of C (but the first) whose cc is not (cc of the member in front
 *               + 1) & 15 and whose discontinuity_indicator is 0.  A duplicate packet (same cc twice, which the standard
 *               allows a muxer to send) therefore counts as a break AND is copied like any other member: duplicates are
 *               not dropped;
 *               reserved[2] = skipped packets (HBS_TS_SKIPPED at or behind the first PES start, and all in front of it).
 *               error = HBS_E_ARG on any fault: reserved[0] = 1 + the lowest faulty packet number, the counts mean
 *               nothing.  Else error = HBS_E_CAPACITY when out_cap is below the output or, with d_pes, pes_cap is below
 *               the PES count; the counts are right.  On either error nothing is written to d_out or d_pes.
 * Nothing outside [d_out, d_out + output bytes) and d_pes[0, PES count) is stored; no load touches a 16-byte granule that
 * holds no byte of d_ts[0, ts_bytes); no host synchronisation.  Alignment: d_ts, d_out, d_summary 16 bytes; d_pes 8 bytes.
 * Not done: PES headers continued in a following packet, dropping duplicates, resynchronising after
 * sync loss, PSI on the device, several PIDs in one call, PCR.
 */
#define HBS_TS_FAULT      (-1)
#define HBS_TS_OTHER        0
#define HBS_TS_SKIPPED      1
#define HBS_TS_NO_PAYLOAD   2
#define HBS_TS_PAYLOAD      3
#define HBS_TS_PES_START    4
#define HBS_TS_PTS            1u   /* flags of hbs_ts_pes / hbs_ts_packet: a PTS is present  */
#define HBS_TS_DTS            2u   /* a DTS is present                                        */
#define HBS_TS_RANDOM_ACCESS  4u   /* random_access_indicator of the packet                   */
#define HBS_TS_DISCONTINUITY  8u   /* discontinuity_indicator of the packet                   */
#define HBS_TS_DATA_ALIGNED  16u   /* data_alignment_indicator of the PES header (q[6] & 4)   */

typedef struct hbs_ts_pes {   /* 32 bytes */
    uint64_t out_off;  /* output offset of the first ES byte of this PES packet */
    uint64_t pts;      /* 33 bits; ~0 when absent */
    uint64_t dts;      /* the DTS; = pts when only a PTS is present; ~0 when neither */
    uint32_t packet;   /* number of the transport packet it begins in */
    uint32_t flags;    /* HBS_TS_PTS | HBS_TS_DTS | HBS_TS_RANDOM_ACCESS | HBS_TS_DISCONTINUITY | HBS_TS_DATA_ALIGNED */
} hbs_ts_pes;

int hbs_ts_demux(hbs_ctx* ctx, const uint8_t* d_ts, uint64_t ts_bytes, int packet_bytes, int pid,
                 uint8_t* d_out, uint64_t out_cap, hbs_ts_pes* d_pes, uint64_t pes_cap, hbs_summary* d_summary);

/*
 * Host side, plain C, no GPU involved.
 * hbs_ts_packet_host: the packet rule above for ONE packet of packet_bytes bytes in host memory -- the very function the
 * kernels run (csrc/hbs_ts.h).  off / es_off count from transport byte 0 (add 4 for the position inside a 192-byte
 * packet).  A fault leaves everything but cls and pid at 0 (pts, dts: ~0).  Returns 0, or HBS_E_ARG (null pointer,
 * packet_bytes, pid).
 * hbs_ts_find_pid_host: the PID of the first elementary stream of `stream_type` (0x24: HEVC) in the first program of a
 * transport stream's head: the first PAT section (PID 0, payload_unit_start, behind its pointer_field, table_id 0), its first
 * entry with program_number != 0 (whose PID carries the PMT; *program_out = that number, when not NULL), the first
 * section with table_id 2 on that PID.  -1 when it is not found or a section does not lie inside one packet.  CRCs are not
 * checked; every length read from the buffer is bounded against the packet before it is used; bytes behind the last whole
 * packet are not read.
 */
typedef struct hbs_ts_packet {   /* 48 bytes */
    int32_t  cls;             /* HBS_TS_*                                                         */
    uint32_t pid;
    uint32_t off, len;        /* the payload b[off, off + len)                                     */
    uint32_t es_off, es_len;  /* its ES bytes b[es_off, es_off + es_len)                           */
    uint32_t cc;              /* continuity_counter                                                */
    uint32_t flags;           /* as hbs_ts_pes.flags                                               */
    uint64_t pts, dts;        /* as hbs_ts_pes                                                     */
} hbs_ts_packet;
int hbs_ts_packet_host(const uint8_t* packet, int packet_bytes, int pid, hbs_ts_packet* out);
int hbs_ts_find_pid_host(const uint8_t* bytes, uint64_t n, int packet_bytes, int stream_type, int* program_out);

/*
 * ---- access units -> MPEG transport stream packets, PES times, PAT / PMT -----------------------------------------------
 * hbs_ts_mux is the way back: every access unit of an Annex-B stream in device memory becomes one PES packet, cut into
 * transport packets of one PID, with a PAT and a PMT where asked for.  hbs_ts_demux of the output returns the AUs' bytes back
 * to back, their times, and RANDOM_ACCESS on the IRAP AUs.
 *
 * ES BYTES OF AU a.  stream[unit_begin_a, unit_end_a), E of them (E may be 0).  Of d_au only unit_begin, unit_end and
 * flags & HBS_AU_IRAP are read; AUs need not touch.  An entry is well-formed when unit_begin <= unit_end <= stream_bytes and
 * unit_begin_a >= unit_end_{a-1}; so a GOP cut is muxed by passing d_au + first, with no filter pass in between.
 * TIMES.  pts = d_pts[a], dts = d_dts ? d_dts[a] : ~0; ~0 means absent, every other value must be below 2^33, a DTS without a
 * PTS is an error.  f = 3 when a DTS is present and differs from the PTS, 2 when a PTS is present and f is not 3, else 0.
 * d_pts == NULL: no AU has a PTS.
 * PES HEADER.  00 00 01 E0 00 00 84 (f << 6) (H - 9), then the time bytes: H = 9, 14 or 19.  PES_packet_length is 0 (legal
 * for video in a transport stream).  A time t is the five bytes
 *   marker << 4 | ((t >> 30) & 7) << 1 | 1,  t >> 22,  ((t >> 15) & 0x7F) << 1 | 1,  t >> 7,  (t & 0x7F) << 1 | 1
 * (each modulo 256), the marker 2 for a PTS alone, 3 for the PTS of a pair, 1 for the DTS.
 * PACKETS OF AU a.  T = H + E.  The first packet always carries an adaptation field: its length byte, a flags byte (0x40 if
 * IRAP, 0x10 if PCR) and, with a PCR, the six bytes base >> 25, base >> 17, base >> 9, base >> 1, (base & 1) << 7 | 0x7E, 0
 * with base = ((f == 3 ? dts : pts) - pcr_lead) mod 2^33.  A PCR is present iff HBS_TSMUX_PCR is set and f != 0.  That is
 * A1 = 2 or 8 bytes, and R1 = 184 - A1.  If T <= R1 the AU is one packet with adaptation_field_length 183 - T, FF stuffing
 * behind the flags and the PCR.  Otherwise the first packet carries R1 bytes with adaptation_field_length A1 - 1 and the rest
 * goes 184 bytes to a packet; only the last of these may be short: with r bytes, 1 <= r < 184, its
 * adaptation_field_length is 183 - r -- a flags byte 00 and then FF when that is >= 1, the length byte alone when it is 0.
 * N(a) = 1 + ceil((T - R1) / 184) packets (1 when T <= R1): what hbs_ts_mux_au_packets_host returns.
 * TRANSPORT HEADER.  47, pusi << 6 | pid >> 8, pid & 0xFF, afc << 4 | cc: pusi on an AU's first packet, afc 3 with an
 * adaptation field, else 1, cc = (cc_es + j) & 15 for the j-th ES packet of the call.
 * PSI.  A PAT packet and then a PMT packet stand in front of AU 0 unless HBS_TSMUX_NO_PSI is set, and with
 * HBS_TSMUX_PSI_AT_IRAP also in front of every later AU with HBS_AU_IRAP (HBS_TSMUX_NO_PSI wins over it).  The k-th pair
 * (from 0) carries cc = (cc_pat + k) & 15 and (cc_pmt + k) & 15.  Both packets are 47 40|pid>>8 pid&FF 10|cc, a
 * pointer_field 0, the section, then FF to byte 188:
 *   PAT section   00 B0 0D tsid(2) C1 00 00 program(2) E0|pmt_pid>>8 pmt_pid&FF crc(4)                       (on PID 0)
 *   PMT section   02 B0 18 program(2) C1 00 00 E0|pid>>8 pid&FF F0 00 24 E0|pid>>8 pid&FF F0 06 05 04 'H' 'E' 'V' 'C' crc(4)
 *                 (on pmt_pid; the PCR PID is the ES PID)
 * crc = MPEG-2 CRC-32 of the section in front of it: polynomial 0x04C11DB7, initial value 0xFFFFFFFF, not reflected, no
 * final xor, most significant byte first.  hbs_ts_mux_psi_host writes the pair with k = 0; the call builds it once and hands
 * it to the kernel by value, the device patches the cc nibble.
 *
 * THE CALL.  The output is those packets in that order, packet_bytes each: with 192 four zero bytes stand in front of the
 * 188, with 204 sixteen behind.  d_au_packet[a] (optional, n_aus + 1 entries) = the number of the packet AU a's PES begins
 * in -- PSI packets count, so an AU behind a pair begins two packets later -- and entry n_aus the total.
 * d_out == NULL: plan only, the summary alone is written.  n_aus == 0 is valid (no packet at all).
 *   d_summary   nal_count = packets, nal_found = n_aus, rbsp_bytes = ES bytes carried, stream_bytes = output bytes,
 *               stop_reason = 0, reserved[1] = ES packets (the next call's cc_es is (cc_es + reserved[1]) & 15),
 *               reserved[2] = PSI pairs.
 *               error = HBS_E_ARG when an AU entry is malformed, a time rule is broken (reserved[0] = 1 + the lowest such
 *               AU; the counts mean nothing) or the call has more than 2^32 - 1 packets (reserved[0] = 0).  Else
 *               HBS_E_CAPACITY when out_cap is below the output; the counts are right.  On either error nothing is written
 *               to d_out or d_au_packet.
 * Refused with HBS_E_ARG at once, before anything is written: params NULL or out of range (packet_bytes not 188 / 192 / 204,
 * a PID outside 16..8190 or pid == pmt_pid, program_number outside 1..65535, transport_stream_id outside 0..65535, unknown
 * flags, a continuity counter above 15, reserved != 0), n_aus above 2^32 - 1, misaligned pointers.
 * Nothing outside [d_out, d_out + output bytes) and d_au_packet[0, n_aus] is stored; no load touches a 16-byte granule that
 * holds no byte of the stream; no host synchronisation; scratch comes from the context's workspace (8 bytes an AU, and 4 bytes
 * per 2048 packets of what out_cap and the stream can hold).
 * Alignment: d_stream, d_out, d_au, d_summary 16 bytes; d_pts, d_dts 8 bytes; d_au_packet 4 bytes.
 * STATED LIMITS: one AU to one PES packet; one PID; no null-packet padding to a constant bitrate; no access-unit delimiters
 * are inserted (13818-1 wants one per HEVC AU: hbs_au_insert adds them, and its d_au_out is this call's d_au); no descriptors
 * beyond the registration descriptor.
 *
 * Host side, plain C, no GPU involved.
 * hbs_ts_mux_psi_host: the PAT and PMT packets of the first pair (188 transport bytes each).  0, or HBS_E_ARG (a NULL
 * pointer, params out of range).
 * hbs_ts_mux_au_packets_host: N(a) for es_bytes ES bytes; time_fields 0: no time, 1: a PTS, 2: a PTS and a DTS that differs;
 * pcr non-zero: HBS_TSMUX_PCR is set (it adds nothing to an AU without a time).  0 for another time_fields.
 */
typedef struct hbs_ts_mux_params {   /* HOST memory, 48 bytes */
    int32_t  packet_bytes;        /* 188, 192 (4 zero bytes in front of each packet) or 204 (16 zero bytes behind) */
    int32_t  pid, pmt_pid;        /* 16..8190, different from each other */
    int32_t  program_number;      /* 1..65535 */
    int32_t  transport_stream_id; /* 0..65535 */
    uint32_t flags;               /* HBS_TSMUX_* */
    uint32_t cc_es, cc_pat, cc_pmt; /* continuity counters of the first packet of each PID, 0..15 */
    uint32_t reserved;            /* 0 */
    uint64_t pcr_lead;            /* 90 kHz ticks the PCR runs behind the DTS */
} hbs_ts_mux_params;
#define HBS_TSMUX_PCR          1u  /* a PCR in the first packet of every AU that has a time */
#define HBS_TSMUX_PSI_AT_IRAP  2u  /* PAT + PMT also in front of every AU with HBS_AU_IRAP */
#define HBS_TSMUX_NO_PSI       4u  /* no PAT / PMT at all (a segment that continues another) */

struct hbs_access_unit;            /* hbs_access_units' record, below */
int hbs_ts_mux(hbs_ctx* ctx, const uint8_t* d_stream, uint64_t stream_bytes,
               const struct hbs_access_unit* d_au, uint64_t n_aus,
               const uint64_t* d_pts, const uint64_t* d_dts /* nullable */,
               const hbs_ts_mux_params* params,
               uint8_t* d_out, uint64_t out_cap,
               uint32_t* d_au_packet /* optional, n_aus + 1 */, hbs_summary* d_summary);
int hbs_ts_mux_psi_host(const hbs_ts_mux_params* params, uint8_t pat188[188], uint8_t pmt188[188]);
uint64_t hbs_ts_mux_au_packets_host(uint64_t es_bytes, int time_fields /* 0, 1, 2 */, int pcr);

/*
 * ---- NAL units -> RTP packets (RFC 7798): single NAL unit packets, fragmentation units, the marker bit ------------------
 * hbs_rtp_pack is the third transport: every NAL of a stream in device memory becomes one RTP packet, or a run of
 * fragmentation units (FUs) when it is larger than a packet may be.  It needs the stream, its index and, for the marker bit and
 * the timestamps, the AU number of every NAL (hbs_access_units' d_nal_au, hbs_au_insert's d_nal_au_out) and the AUs' times
 * (hbs_ts_demux's PES table).
 *
 * NAL k.  Bytes stream[start_k, end_k), L = end - start; h0 = stream[start], h1 = stream[start + 1], type t = (h0 >> 1) & 63;
 * mp = max_payload, F = mp - 3.
 * SINGLE NAL UNIT PACKET, when L <= mp: one packet whose payload is the L bytes verbatim.
 * FRAGMENTATION UNITS, when L > mp: the body is the B = L - 2 bytes stream[start + 2, end); n = ceil(B / F) packets (always
 * >= 2, so no FU carries both S and E).  Packet i carries the 2-byte PayloadHdr (h0 & 0x81) | 0x62, h1 (type 49, the NAL's F
 * bit, layer id and TID), then the FU header (i == 0) << 7 | (i == n - 1) << 6 | t, then the body bytes
 * [i F, min((i + 1) F, B)): only the last fragment is short.  No DONL fields (sprop-max-don-diff = 0).
 * RTP HEADER, 12 bytes.  0x80, M << 7 | payload_type, the sequence number (seq + j) & 0xFFFF of the call's j-th packet
 * big-endian, the timestamp big-endian, the ssrc big-endian.  M = 1 exactly on the last packet of the last NAL of an access
 * unit: NAL k with k == n_nals - 1 or d_nal_au[k + 1] != d_nal_au[k]; with HBS_RTP_OPEN_END the call's last NAL is exempt.
 * AGGREGATION PACKETS (RFC 7798 4.4.2), with HBS_RTP_AGGREGATE only; without the flag every byte of output, every table entry
 * and the summary are what they are without this paragraph.  The call's NALs are cut into GROUPS of consecutive NALs, greedily:
 * next(i) is the smallest j > i with j == n_nals, j % HBS_RTP_AP_SPAN == 0, a_j != a_i or 2 + sum_{m = i..j} (2 + L_m) > mp; the
 * group starts are g_0 = 0 and g_{r+1} = next(g_r).  The cut at every multiple of HBS_RTP_AP_SPAN (256) in the call's NAL
 * numbering is part of the definition: it costs at most one packet more per 256 NALs, no plan workgroup waits for another
 * because of it, and a call split at a multiple of 256 NALs makes the same packets.  A group never crosses an access unit, so
 * its NALs share one timestamp.  A group of one NAL is sent as above (single NAL unit packet or FUs).  A group of m >= 2 NALs is
 * ONE aggregation packet: the RTP header, the 2-byte PayloadHdr F << 7 | 48 << 1 | layer >> 5, (layer & 31) << 3 | tid with F the
 * OR of (h0 >> 7), layer the lowest (h0 & 1) << 5 | h1 >> 3 and tid the lowest h1 & 7 of its NALs, then for each NAL in order a
 * big-endian 16-bit L and its L bytes verbatim.  No DONL fields.  For mp < 10 no AP can exist.  M = 1 on an AP exactly when its
 * last unit ends its access unit (HBS_RTP_OPEN_END exempts the call's last NAL here too); an AP takes one sequence number.
 * The output is never larger than without the flag: an AP of m units saves (m - 1)(framing + 12) - 2 - 2m >= 6 bytes.
 * ACCESS UNITS AND TIMES.  a_k = d_nal_au[k] - d_nal_au[0]; every step d_nal_au[k] - d_nal_au[k - 1] must be 0 or 1 and
 * a_k < n_aus, so a range is passed by pointer offset into the tables, like a GOP cut to hbs_ts_mux.  d_nal_au == NULL: the
 * whole batch is AU 0 and n_aus is ignored.  The timestamp of AU a, modulo 2^32, is ts_base + (uint32_t)d_pts[a] when d_pts is
 * given and ts_base + a * ts_step when it is not.  A d_pts[a] of 2^33 or more is an error, the ~0 "absent" of hbs_ts_demux
 * included: RTP has no packet without a time.
 *
 * THE CALL.  The output is the packets of NAL 0, 1, ... in that order, each as `framing` bytes of length (12 + payload bytes,
 * big-endian; RFC 4571) when framing is 2, the header, the payload.  Nothing between NALs is copied.  d_nal_off[k] (optional,
 * n_nals + 1 entries) = the output offset where NAL k's first packet begins, its length field included, entry n_nals the
 * total; d_nal_packet[k] (optional, n_nals + 1) = the number of NAL k's first packet, entry n_nals the packet count.  All
 * packets of a NAL but its last take framing + 12 + mp bytes, so the two tables and the rule give every packet's offset
 * without a table per packet.  With HBS_RTP_AGGREGATE the NALs of an AP share a packet: d_nal_packet[k] = the number of the
 * packet that carries NAL k's first byte, the same for all units of an AP; d_nal_off[k] = where NAL k's share of the output
 * begins -- for the first NAL of a packet the packet's beginning (length field included), for a later unit of an AP its 16-bit
 * size field.  Packet p begins at d_nal_off of the first k with d_nal_packet[k] == p.  d_out == NULL: plan only, the summary alone is written.  n_nals == 0 is valid: an empty output,
 * entry 0 of both tables 0.
 *   d_summary   nal_count = packets, nal_found = n_nals, rbsp_bytes = NAL bytes carried (the sum of L), stream_bytes = output
 *               bytes, stop_reason = 0, reserved[1] = packets (the next call's seq is (seq + reserved[1]) & 0xFFFF),
 *               reserved[2] = aggregation packets << 32 | NALs sent as FUs (the high word is 0 without HBS_RTP_AGGREGATE).
 *               error = HBS_E_ARG with reserved[0] = 1 + the lowest offending NAL when a NAL has L < 2, has t >= 48 (48 to 50
 *               mean AP / FU / PACI to a receiver: filter such NALs out first with hbs_filter_annexb), has an index entry that
 *               is inconsistent by the filter's definition (start > end, end > stream_bytes, start_k < end_{k-1}), breaks an
 *               AU-number rule or belongs to an AU whose time is out of range; every record is checked before it is used;
 *               the other counts mean nothing then.  Else HBS_E_CAPACITY when out_cap is below the output; the counts are
 *               right.  On either error nothing is written but the summary.
 * Refused with HBS_E_ARG at once, before anything is written: params NULL or out of range (max_payload outside 4..65523,
 * payload_type outside 0..127, framing not 0 or 2, flags other than HBS_RTP_OPEN_END | HBS_RTP_AGGREGATE, seq above 65535), n_nals above 2^32 - 1, out_cap above 2^46
 * with a d_out, missing or misaligned pointers.
 * Nothing outside [d_out, d_out + output bytes), the n_nals + 1 entries of the two tables and the summary is stored; no load
 * touches a 16-byte granule that holds no byte of the stream, and a NAL's first byte is read only after its entry has been
 * checked; no host synchronisation; scratch comes from the context's workspace (40 bytes a NAL, 44 with HBS_RTP_AGGREGATE, and 8 bytes per
 * 64 KiB output tile of what out_cap and the stream can hold).
 * Alignment: d_stream, d_out, d_summary 16 bytes; d_index, d_pts, d_nal_off, d_nal_packet 8 bytes; d_nal_au 4 bytes.
 * STATED LIMITS: no DONL fields, no interleaving; no PACI; no header extension and no CSRC entries on the sending side; no
 * RTCP; no SRTP.  The way back is hbs_rtp_unpack (below), which reads the output with and without HBS_RTP_AGGREGATE;
 * hbs_rtp_packet_host reads one packet on the host and hbs_rtp_ap_units_host the units of an aggregation packet.
 *
 * Host side, plain C, no GPU involved.
 * hbs_rtp_nal_packets_host: the packets of a NAL of nal_bytes bytes; 0 for nal_bytes < 2 or a max_payload out of range.
 * hbs_rtp_packet_host: one RTP packet pkt[0, n) (without a length field) as a receiver reads it -- CSRC entries, a header
 * extension and padding are accounted for by RFC 3550, so payload_off / payload_len are right for packets this library did not
 * write.  kind by the payload's type: below 48 a single NAL unit (nal_off / nal_len = the payload), 49 an FU (fu_start,
 * fu_end, nal_type from the FU header, nal_header = the two reconstructed header bytes of the NAL, nal_off / nal_len = the
 * fragment behind the three bytes), 48 an AP, anything else HBS_RTP_OTHER (a payload below 2 bytes: nal_type -1).  0, or
 * HBS_E_ARG for a version other than 2, NULL pointers or a packet shorter than its own fields say.
 * hbs_rtp_ap_units_host: the units of the aggregation packet pkt[0, n) (without a length field): returns their count and fills
 * the offset within pkt and the size of the first `cap` of them (off_out and size_out may be NULL when cap is 0).  HBS_E_ARG when
 * hbs_rtp_packet_host refuses the packet, when its kind is not HBS_RTP_AP, or when rule 4 of hbs_rtp_unpack (below) calls it a
 * fault: no unit, a size that does not fit, a size below 2, a unit of type 48 or above.  No size is used before it is bounded.
 */
typedef struct hbs_rtp_params {   /* HOST memory, 32 bytes */
    int32_t  max_payload;   /* most RTP payload bytes in a packet (behind the 12-byte header): 4 .. 65523 */
    int32_t  payload_type;  /* 0 .. 127 */
    int32_t  framing;       /* 0: packets back to back; 2: a big-endian 16-bit packet length in front of each (RFC 4571) */
    uint32_t flags;         /* HBS_RTP_* */
    uint32_t ssrc;
    uint32_t seq;           /* sequence number of the call's first packet, 0 .. 65535 */
    uint32_t ts_base;       /* added to every timestamp, modulo 2^32 */
    uint32_t ts_step;       /* with d_pts == NULL: the timestamp of AU a is ts_base + a * ts_step */
} hbs_rtp_params;
#define HBS_RTP_OPEN_END 1u  /* the call's last NAL does not end its access unit: no marker bit on its last packet */
#define HBS_RTP_AGGREGATE 4u /* consecutive small NALs of an access unit share an aggregation packet                  */
#define HBS_RTP_AP_SPAN 256  /* ... and no aggregation packet reaches across a multiple of this in the call's NAL numbering */

#define HBS_RTP_SINGLE 0     /* hbs_rtp_packet.kind */
#define HBS_RTP_FU     1
#define HBS_RTP_AP     2
#define HBS_RTP_OTHER  3
typedef struct hbs_rtp_packet {   /* 72 bytes */
    uint64_t payload_off, payload_len;   /* the RTP payload: behind header, CSRC entries and extension, in front of the padding */
    uint64_t nal_off, nal_len;           /* where the NAL's bytes lie (an FU: the fragment)                                     */
    int32_t  kind;                       /* HBS_RTP_SINGLE / FU / AP / OTHER                                                    */
    int32_t  nal_type;                   /* the NAL's type (an FU: from the FU header); -1: no payload header                   */
    uint32_t marker, payload_type, seq, timestamp, ssrc;
    uint32_t fu_start, fu_end;           /* an FU's S and E bits                                                                */
    uint8_t  nal_header[2];              /* the NAL's two header bytes (an FU: reconstructed)                                   */
    uint8_t  reserved[2];
} hbs_rtp_packet;

int hbs_rtp_pack(hbs_ctx* ctx, const uint8_t* d_stream, uint64_t stream_bytes,
                 const hbs_nal_entry* d_index, uint64_t n_nals,
                 const uint32_t* d_nal_au /* nullable */, uint64_t n_aus, const uint64_t* d_pts /* nullable */,
                 const hbs_rtp_params* params,
                 uint8_t* d_out, uint64_t out_cap,
                 uint64_t* d_nal_off /* optional, n_nals + 1 */, uint64_t* d_nal_packet /* optional, n_nals + 1 */,
                 hbs_summary* d_summary);
uint64_t hbs_rtp_nal_packets_host(uint64_t nal_bytes, int max_payload);
int hbs_rtp_packet_host(const uint8_t* pkt, uint64_t n, hbs_rtp_packet* out);
int64_t hbs_rtp_ap_units_host(const uint8_t* pkt, uint64_t n, uint64_t* off_out, uint64_t* size_out, uint64_t cap);

/*
 * ---- RTP packets (RFC 7798) -> Annex-B: single NAL unit packets, aggregation packets, fragmentation units ---------------
 * hbs_rtp_unpack is the receiver's side of the third transport: a table of RTP packets in device memory becomes the Annex-B
 * stream of their NAL units, with the index hbs_parse_headers* and hbs_filter_annexb take, the AU number of every NAL and the
 * timestamp of every AU.  hbs_rtp_pack makes aggregation packets only with HBS_RTP_AGGREGATE; this call reads them either way.
 *
 * PACKETS.  Packet p is d_in[d_pkt_off[p], d_pkt_off[p] + d_pkt_size[p]), a raw RTP packet without a length field.  Packets may
 * lie anywhere in the buffer, in any order, and may overlap, like the samples of hbs_lenpref_to_annexb; the output follows the
 * order of the TABLE, so a caller reorders late packets by permuting the table.  The framed output of hbs_rtp_pack (framing 2)
 * is passed by adding 2 to each packet offset; hbs_rtp_frames_host makes the table of any RFC 4571 byte stream.
 *
 * THE PACKET RULE, in this order.
 * 1. ENTRY FAULT: off + size wraps or exceeds in_bytes.  Every entry is checked before a byte of its packet is read.
 * 2. HEADER FAULT: what hbs_rtp_packet_host refuses -- fewer than 12 bytes, a version other than 2, shorter than its own CSRC /
 *    extension / padding fields say, a fragmentation unit's payload below 3 bytes.  (One function, rtp_packet_rule, runs in the
 *    kernels and behind hbs_rtp_packet_host.)
 * 3. OTHER: the payload type differs from params->payload_type, or, with HBS_RTPU_MATCH_SSRC, the ssrc differs from
 *    params->ssrc.  Such a packet is not this stream's and plays no further part, but it still stands between its table
 *    neighbours: it ends a chain (below) and no sequence break is counted across it.
 * 4. ACCEPTED, by the type t = (payload[0] >> 1) & 63 of the payload's first two bytes (the PayloadHdr):
 *    a payload below 2 bytes, or t in 50..63 (PACI, reserved): unsupported -- dropped and counted;
 *    t < 48: a single NAL unit, the payload verbatim;
 *    t == 48: an aggregation packet without DONL fields.  Behind the PayloadHdr come units of a big-endian 16-bit size s and
 *      then s bytes, until the payload's end; each unit is one NAL.  A FAULT when there is no unit, when fewer than 2 bytes are
 *      left for a size, when s < 2 or s exceeds what is left, or when a unit's NAL type is 48 or above.  Every size is bounded
 *      before it is used;
 *    t == 49: a fragmentation unit (FU): PayloadHdr, the FU header S << 7 | E << 6 | type, the fragment.  A FAULT when the FU
 *      header's type is 48 or above.  An empty fragment is accepted; S and E both set is a NAL of one fragment.
 * CHAINS.  An accepted FU p CONTINUES packet p - 1 of the table when p has no S, p - 1 is an accepted FU without E, both have
 * the same FU type, the same two PayloadHdr bytes, the same timestamp and the same ssrc, and seq_p == (seq_{p-1} + 1) & 0xFFFF.
 * A chain is a maximal run of FUs in which every packet but the first continues the one in front of it; it is WHOLE when its
 * first packet has S and its last has E.  A whole chain is one NAL: the two header bytes (payload[0] & 0x81) | type << 1,
 * payload[1] rebuilt from its first packet, then the fragments in order; its timestamp is its first packet's and its marker its
 * last packet's.  Every FU of a chain that is not whole is dropped and counted: ONLY WHOLE NALS EVER REACH THE OUTPUT.
 *
 * THE OUTPUT.  For every NAL in table order `startcode_bytes` bytes of start code (00 00 01 or 00 00 00 01) and then its bytes.
 * d_index_out[k] (optional): start / end = NAL k's bytes in the output (behind its start code), rbsp_off = rbsp_len = 0,
 * status = 0 and HBS_ST_UNTERMINATED on the last entry only -- what hbs_index_extract says of the same stream.
 * ACCESS UNITS.  NAL k begins an access unit when k == 0, when its timestamp differs from NAL k - 1's, or when NAL k - 1
 * carried the marker; the marker of an aggregation packet belongs to its last unit.  d_nal_au_out[k] (optional) = the AU's
 * number from 0; d_au_ts_out[a] (optional) = the timestamp of AU a's first NAL as a uint64_t.  The two tables go straight into
 * hbs_rtp_pack, hbs_ts_mux (as its times) and hbs_annexb_to_lenpref.
 * d_out == NULL: plan only -- the summary alone is written and no capacity is looked at.  n_packets == 0 is valid.
 *   d_summary   nal_count = NALs, nal_found = accepted packets, stream_bytes = output bytes, rbsp_bytes = NAL bytes (the output
 *               without its start codes), stop_reason = -1 when a NAL came out, else 0; reserved[1] = access units;
 *               reserved[2] = sequence breaks << 32 | dropped packets.  A sequence break is a pair of table neighbours, both
 *               accepted, with seq_p != (seq_{p-1} + 1) & 0xFFFF.  A dropped packet is an accepted packet of which no byte
 *               reaches the output: an unsupported one, or an FU of a chain that is not whole (an empty fragment of a whole
 *               chain is part of its NAL and is not counted).
 *               On any fault error = HBS_E_ARG and reserved[0] = 1 + the lowest faulty packet; the other counts mean nothing
 *               (they are 0).  Else HBS_E_CAPACITY when, with a d_out, the output exceeds out_cap, the NALs exceed nal_cap or,
 *               with a d_au_ts_out, the access units exceed au_cap; the counts are right then.  On either error nothing but
 *               the summary is written.
 * Refused with HBS_E_ARG at once, before anything is written: params NULL or out of range (payload_type outside 0..127,
 * startcode_bytes not 3 or 4, unknown flags), n_packets above 2^32 - 1, out_cap above 2^46 with a d_out, missing or misaligned
 * pointers (with packets: the two tables, and d_in when in_bytes is not 0).
 * Nothing outside [d_out, d_out + output bytes), the first nal_count entries of d_index_out and d_nal_au_out, the first
 * reserved[1] entries of d_au_ts_out and the summary is stored; no load touches a 16-byte granule that holds no byte of
 * d_in[0, in_bytes); no host synchronisation; scratch comes from the context's workspace and is sized by n_packets, nal_cap
 * and out_cap alone (44 bytes a packet, 24 bytes a piece of at most n_packets + min(nal_cap, out_cap / (startcode_bytes + 2))
 * pieces, 8 bytes per 64 KiB of out_cap).
 * Alignment: d_in, d_out, d_summary 16 bytes; d_pkt_off, d_pkt_size, d_index_out, d_au_ts_out 8 bytes; d_nal_au_out 4 bytes.
 * STATED LIMITS: no reordering and no duplicate removal beyond the table's order (a duplicate comes out twice and counts as a
 * break): hbs_rtp_order (below) makes the table of a receiver's arrival order that this call reads; no DONL fields, no interleaving; no PACI; a packet that is not this stream's and lies inside a chain breaks the
 * chain; no RTCP; no SRTP.
 *
 * Host side, plain C, no GPU involved.
 * hbs_rtp_frames_host walks an RFC 4571 byte stream bytes[0, n): a big-endian 16-bit length, then a packet of that many bytes,
 * and so on.  It stops in front of the first incomplete frame; no length is trusted before it is bounded.  Returns the number
 * of whole frames and fills the offset / size (of the packets, the length fields left out) of the first `cap` of them;
 * *used_out = the bytes the whole frames take, where the next read continues.  off_out, size_out and used_out may be NULL.
 */
typedef struct hbs_rtp_unpack_params {   /* HOST memory, 16 bytes */
    int32_t  payload_type;      /* 0 .. 127: packets of another type are not this stream's */
    int32_t  startcode_bytes;   /* 3: 00 00 01, 4: 00 00 00 01 in front of every NAL */
    uint32_t flags;             /* HBS_RTPU_* */
    uint32_t ssrc;              /* read with HBS_RTPU_MATCH_SSRC */
} hbs_rtp_unpack_params;
#define HBS_RTPU_MATCH_SSRC 1u  /* packets whose ssrc differs from params->ssrc are not this stream's */

int hbs_rtp_unpack(hbs_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes,
                   const uint64_t* d_pkt_off, const uint64_t* d_pkt_size, uint64_t n_packets,
                   const hbs_rtp_unpack_params* params,
                   uint8_t* d_out, uint64_t out_cap,
                   hbs_nal_entry* d_index_out /* optional */, uint32_t* d_nal_au_out /* optional */, uint64_t nal_cap,
                   uint64_t* d_au_ts_out /* optional */, uint64_t au_cap,
                   hbs_summary* d_summary);
uint64_t hbs_rtp_frames_host(const uint8_t* bytes, uint64_t n, uint64_t* off_out, uint64_t* size_out, uint64_t cap,
                             uint64_t* used_out);

/*
 * ---- RTP packets in arrival order -> the table hbs_rtp_unpack reads: by sequence number, without duplicates ---------------
 * hbs_rtp_order is the jitter-buffer step in front of hbs_rtp_unpack: a table of RTP packets in the order a receiver got them
 * -- late packets, duplicates, 16-bit sequence numbers that wrap -- becomes the table of the same packets in the sender's
 * order, each once.  No packet byte is moved: the output is a permutation of a subset of the input table's entries.
 *
 * PACKETS are table entries exactly as hbs_rtp_unpack takes them: packet p is d_in[d_pkt_off[p], d_pkt_off[p] + d_pkt_size[p]),
 * anywhere in d_in, in any order, overlapping allowed.  The TABLE order is the arrival order.
 *
 * THE RULE, in this order.
 * 1. ENTRY FAULT and HEADER FAULT: steps 1 and 2 of hbs_rtp_unpack's packet rule, by the same function (rtp_packet_rule): off +
 *    size wraps or exceeds in_bytes; fewer than 12 bytes, a version other than 2, shorter than its own CSRC / extension / padding
 *    fields say, a fragmentation unit's payload below 3 bytes.  Any fault: error = HBS_E_ARG and reserved[0] = 1 + the lowest
 *    faulty entry, the other counts are 0 and nothing but the summary is written.  Every entry is bounded before a byte of its
 *    packet is read.  A table that passes here never produces a header fault in hbs_rtp_unpack (its aggregation packet and FU
 *    type faults look at the payload, which this call does not).
 * 2. OTHER: the payload type differs from params->payload_type, or, with HBS_RTPO_MATCH_SSRC, the ssrc differs from
 *    params->ssrc.  The packet is left out of the output and of the sequence.
 * 3. EXTENDED SEQUENCE NUMBER of the accepted packets (neither faulty nor OTHER) a_0, a_1, ... in TABLE order.  With sext16(x) =
 *    the low 16 bits of x read as a signed number (sext16(0x8000) = -32768):
 *      ext(a_0) = 2^48 + seq(a_0), or, with HBS_RTPO_AFTER, params->after_ext + sext16(seq(a_0) - params->after_ext);
 *      ext(a_i) = ext(a_(i-1)) + sext16(seq(a_i) - seq(a_(i-1))).
 *    With n_packets below 2^32 no value leaves (2^47, 2^49 + 2^48); after_ext must lie in [2^48, 2^62].  (A prefix sum of signed
 *    16-bit differences: no sequential walk.)  The numbers are the sender's whenever any two packets that arrive next to each
 *    other lie fewer than 2^15 apart in the sender's order; the call cannot see where that does not hold.
 * 4. LATE (with HBS_RTPO_AFTER only): ext <= params->after_ext.  The packet is dropped.
 * 5. DUPLICATE: an accepted packet that is not late and whose ext equals that of an accepted, not late packet earlier in the
 *    table.  It is dropped: the first arrival wins.  Contents are not compared.
 * 6. KEPT: every other accepted packet.
 *
 * THE OUTPUT.  The kept packets in ascending ext: d_off_out[k] / d_size_out[k] are copied from the packet's input entry,
 * d_src_out[k] (optional) is that entry's table position, d_ext_out[k] (optional) its ext.  d_off_out and d_size_out go into
 * hbs_rtp_unpack as its d_pkt_off / d_pkt_size, with the same d_in.
 * SPAN = the highest kept ext - base + 1, where base is the lowest kept ext, or params->after_ext + 1 with HBS_RTPO_AFTER; 0
 * when nothing is kept.  MOVED = the kept packets for which an earlier table entry, accepted and not late, has a higher ext.
 *   d_summary   nal_count = kept packets, nal_found = accepted packets, stream_bytes = span, rbsp_bytes = the highest kept ext
 *               (the next call's after_ext; 0 when nothing is kept), stop_reason = 0; reserved[1] = lost = span - kept (the
 *               sequence numbers inside the span that no packet carried); reserved[2] = duplicates << 32 | moved.  The others
 *               are n_packets - nal_found, the late ones nal_found - nal_count - duplicates.
 *               HBS_E_CAPACITY when span > params->max_span: nal_found and stream_bytes are right, nal_count, rbsp_bytes,
 *               reserved[1] and reserved[2] are 0.  HBS_E_CAPACITY when, with outputs, kept > out_cap: all counts are right.
 *               On any error nothing but the summary is written.
 * d_off_out == d_size_out == NULL: plan only -- the summary alone is written and out_cap is not looked at.  n_packets == 0 is
 * valid.  CHAINING: a receiver calls once per batch with HBS_RTPO_AFTER and after_ext = the rbsp_bytes of the last call that
 * kept a packet; a packet that arrives behind the batch its number belongs to is LATE there.
 * Refused with HBS_E_ARG at once, before anything is written: params NULL or out of range (payload_type outside 0..127, unknown
 * flags, reserved != 0, max_span outside 1..2^33, with HBS_RTPO_AFTER an after_ext outside [2^48, 2^62]), n_packets above
 * 2^32 - 2, one of d_off_out / d_size_out without the other, d_src_out or d_ext_out without them, missing or misaligned pointers
 * (with packets: the two tables, and d_in when in_bytes is not 0).  The outputs may not alias the input tables.
 * Nothing outside the first nal_count entries of the outputs and the summary is stored; no load touches a 16-byte granule that
 * holds no byte of d_in[0, in_bytes); no host synchronisation; scratch comes from the context's workspace and is sized by
 * n_packets and max_span alone: 12 bytes a packet and 168 bytes per 256 packets, 4 bytes a slot (a slot per extended sequence
 * number of max_span) and 64 bytes per 256 slots.  The device work follows the span the call finds, not max_span.
 * Alignment: d_in, d_summary 16 bytes; d_pkt_off, d_pkt_size, d_off_out, d_size_out, d_ext_out 8 bytes; d_src_out 4 bytes.
 * STATED LIMITS: one SSRC's stream a call (HBS_RTPO_MATCH_SSRC picks it); no timing-based release -- the caller decides when a
 * batch is complete; no FEC, no RTX; a duplicate is recognised by its sequence number only.
 */
typedef struct hbs_rtp_order_params {   /* HOST memory, 32 bytes */
    int32_t  payload_type;      /* 0 .. 127: packets of another type are not this stream's */
    uint32_t flags;             /* HBS_RTPO_* */
    uint32_t ssrc;              /* read with HBS_RTPO_MATCH_SSRC */
    uint32_t reserved;          /* 0 */
    uint64_t max_span;          /* 1 .. 2^33: the widest range of extended sequence numbers the call may have to hold */
    uint64_t after_ext;         /* read with HBS_RTPO_AFTER: the extended sequence number of the last packet already delivered */
} hbs_rtp_order_params;
#define HBS_RTPO_MATCH_SSRC 1u  /* packets whose ssrc differs from params->ssrc are not this stream's */
#define HBS_RTPO_AFTER      2u  /* the sequence continues behind params->after_ext; packets at or in front of it are late */

int hbs_rtp_order(hbs_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes,
                  const uint64_t* d_pkt_off, const uint64_t* d_pkt_size, uint64_t n_packets,
                  const hbs_rtp_order_params* params,
                  uint64_t* d_off_out, uint64_t* d_size_out /* both or neither; neither: plan only */,
                  uint32_t* d_src_out /* optional */, uint64_t* d_ext_out /* optional */, uint64_t out_cap /* entries */,
                  hbs_summary* d_summary);

/*
 * K4: header parse, one NAL per lane (64 per wavefront), over the RBSP arena and index that
 * hbs_index_extract produced.  For NAL k it does what read_hevc_nal_unit()
 * does after nal_to_rbsp (hevc_stream.c:175-239): NAL header, then by type the
 * VPS / SPS / PPS / slice-segment-header reader, into structs laid out exactly
 * as hevc_stream.h's (include/hevc_stream.h).  The state the reference threads
 * through one mutable parser object is resolved per NAL: a slice is read
 * against the last SPS and PPS that precede it in the stream.
 *
 *   d_parsed[k]     rc (read_hevc_nal_unit's return value: consumed NAL bytes,
 *                   or -1: bad emulation pattern, unsupported type -- AUD, SEI,
 *                   EOS, ... -- or bit-reader overrun), the hevc_nal_t fields
 *                   (-1 when nal_to_rbsp already failed), where its struct is in
 *                   d_structs, and for slices h->slice_data: payload size and
 *                   where the payload starts inside the NAL's RBSP
 *   d_structs       struct arena: hevc_vps_t / hevc_sps_t / hevc_pps_t /
 *                   hevc_slice_header_t per NAL at d_parsed[k].struct_off
 *                   (an SPS slot is followed by its derived RPS tables);
 *                   NULL = plan only
 *   d_summary       reserved[0] = arena bytes needed; error HBS_E_CAPACITY when
 *                   structs_cap was smaller (NALs that did not fit keep
 *                   struct_off = ~0)
 */
typedef struct hbs_parsed_nal {
    int32_t  rc;
    int32_t  nal_unit_type, nal_layer_id, nal_temporal_id_plus1;
    uint64_t struct_off;
    int32_t  slice_data_size;
    uint32_t slice_data_off;
} hbs_parsed_nal;

int hbs_parse_headers(hbs_ctx* ctx, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                      hbs_parsed_nal* d_parsed, uint8_t* d_structs, uint64_t structs_cap, hbs_summary* d_summary);
/*
 * ---- compact header parse (round 5) -------------------------------------------------------------------------------
 * hbs_parse_headers writes one hevc_slice_header_t per slice: 4 024 bytes, cleared and then filled (reference struct
 * hevc_stream.h:465-515, reader hevc_stream.c:782-941) -- 405 MB for the 100 k NALs of a 4K30 stream, of which a caller that
 * indexes a stream reads a handful of members.  hbs_parse_headers_compact walks every slice header exactly as
 * hbs_parse_headers does (same bits, same order, same derived tables, out-of-spec slices walked again exactly) but WITHOUT a
 * struct: per slice a 64-byte hbs_slice_compact -- sixteen members of hevc_slice_header_t, each equal to the member of the
 * same name in the struct hbs_parse_headers fills -- next to the same hbs_parsed_nal (rc, NAL header, slice_data_off /
 * slice_data_size; struct_off = ~0 for slices).  Parameter sets are parsed into d_structs as always (the slices need them;
 * a VPS + SPS + PPS group is ~0.5 MB).  d_structs = NULL: plan only (d_summary->reserved[0] = arena bytes needed).
 *
 * hbs_parse_materialize is the same call with a list of NAL numbers (device memory, any order): the listed NALs that are
 * slices are walked into full hevc_slice_header_t slots in d_structs behind the parameter sets (d_parsed[k].struct_off says
 * where), every other slice into its compact record as before.  "The full struct on demand": call it with the NALs a caller
 * wants to look at closely; the structs are those of hbs_parse_headers, member for member.
 *
 * No trace and no parser-state output in these calls.  Errors in d_summary->error: HBS_E_CAPACITY (structs_cap), HBS_E_DEPTH
 * (an out-of-spec stream whose exact answer needs the sequential parse: a chain of slice-own RPS sets deeper than three,
 * never seen in 12 000 fuzzed streams; hbs_parse_headers handles it).
 */
typedef struct hbs_slice_compact {
    int32_t first_slice_segment_in_pic_flag, no_output_of_prior_pics_flag, pic_parameter_set_id, dependent_slice_segment_flag;
    int32_t slice_segment_address, slice_type, pic_output_flag, slice_pic_order_cnt_lsb;
    int32_t short_term_ref_pic_set_sps_flag, short_term_ref_pic_set_idx, num_long_term_pics, slice_temporal_mvp_enabled_flag;
    int32_t num_ref_idx_l0_active_minus1, num_ref_idx_l1_active_minus1, slice_qp_delta, num_entry_point_offsets;
} hbs_slice_compact;

int hbs_parse_headers_compact(hbs_ctx* ctx, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                              hbs_parsed_nal* d_parsed, hbs_slice_compact* d_compact, uint8_t* d_structs, uint64_t structs_cap,
                              const uint8_t* d_initial_sps_slot, const uint8_t* d_initial_pps, hbs_summary* d_summary);
int hbs_parse_materialize(hbs_ctx* ctx, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                          hbs_parsed_nal* d_parsed, hbs_slice_compact* d_compact, uint8_t* d_structs, uint64_t structs_cap,
                          const uint8_t* d_initial_sps_slot, const uint8_t* d_initial_pps,
                          const uint64_t* d_nal_list, uint64_t n_list, hbs_summary* d_summary);

/*
 * Opt-in extension: the NAL types read_hevc_nal_unit() returns -1 for without reading them
 * (hevc_stream.c:221-222) -- access unit delimiter 35, end of sequence 36, end of bitstream 37, filler data 38,
 * prefix / suffix SEI 39 / 40 -- read the way the reference's own, never dispatched readers would
 * (read_hevc_access_unit_delimiter_rbsp hevc_stream.c:573-577, read_filler_data_rbsp :590-597, the SEI message loop
 * :524-563 with h264_sei.c's opaque payloads).  Call it behind hbs_parse_headers on the same arrays: for every NAL of
 * those types d_parsed[k].rc becomes the bytes consumed (or -1 when the cursor ran past the RBSP, as :225 does) and
 * d_ext[k] is filled; other NALs' records are zeroed and their d_parsed entries left alone.  hbs_parse_headers by
 * itself keeps the reference's -1.
 */
#define HBS_SEI_MAX_MESSAGES 6
typedef struct hbs_sei_message {
    int32_t  payloadType, payloadSize;     /* sei_t, h264_sei.h:38-47 */
    uint32_t payload_off;                  /* where the payload bytes start inside the NAL's RBSP (not copied) */
    uint32_t reserved;
} hbs_sei_message;
typedef struct hbs_ext_nal {
    int32_t  num_sei_messages;             /* messages the NAL holds; the first HBS_SEI_MAX_MESSAGES are recorded */
    int32_t  primary_pic_type;             /* hevc_aud_t */
    uint32_t filler_bytes;                 /* ff_byte count of a filler data NAL */
    uint32_t reserved;
    hbs_sei_message sei[HBS_SEI_MAX_MESSAGES];
} hbs_ext_nal;
int hbs_parse_extended(hbs_ctx* ctx, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                       hbs_parsed_nal* d_parsed, hbs_ext_nal* d_ext);

/*
 * hbs_index_parse: BASELINE config 3 without an RBSP arena -- find_nal_unit over the whole stream (the index-only scan:
 * start / end / rbsp_off / rbsp_len / status exactly as hbs_index_extract with d_rbsp = NULL), then read_hevc_nal_unit's
 * parse of every NAL, reading each NAL's header straight from the stream: only the bytes the readers can look at are
 * stripped of their emulation prevention bytes (nal_to_rbsp's rule, hevc_stream.c:161-179 / h264_nal.c:147-200) into a
 * small window per NAL -- `header_window` RBSP bytes of a slice segment (0 = 512; 64 ... 65536, a multiple of 16), all of
 * a VPS / SPS / PPS -- instead of the whole stream into an arena.  d_parsed and d_structs come out exactly as from
 * hbs_index_extract + hbs_parse_headers (slice_data_off / slice_data_size still describe the NAL's RBSP, which is not
 * materialised); d_payload_off (optional, one uint64 per NAL) receives the STREAM offset of the first payload byte of
 * every parsed slice (~0 for other NALs).  A slice header that does not end at least 8 bytes inside its window -- hundreds
 * of entry points -- is reported, never guessed: d_parse_summary->error = HBS_E_CAPACITY and that NAL's rc = INT32_MIN;
 * call again with a larger window, or take the arena path.  The call waits once, for the scan's NAL count (returned in
 * *nal_count_out when not NULL); the parse is enqueued behind it.  On the 2.1 GiB 4K30 sequence of bench.py: scan 1 B/B
 * + ~3 % for the windows, against 2 B/B for the arena.
 * Alignment: d_stream, d_parsed, d_structs, both summaries 16 bytes; d_index, d_payload_off 8 bytes.  A misaligned d_structs
 * is refused before the scan runs: no output is written.
 */
int hbs_index_parse(hbs_ctx* ctx, const uint8_t* d_stream, uint64_t stream_bytes,
                    hbs_nal_entry* d_index, uint64_t index_cap, uint32_t header_window,
                    hbs_parsed_nal* d_parsed, uint8_t* d_structs, uint64_t structs_cap, uint64_t* d_payload_off,
                    hbs_summary* d_scan_summary, hbs_summary* d_parse_summary, uint64_t* nal_count_out);
/* the same with the compact parse behind the scan (hbs_parse_headers_compact): d_compact[k] for every NAL, no slice structs */
int hbs_index_parse_compact(hbs_ctx* ctx, const uint8_t* d_stream, uint64_t stream_bytes,
                    hbs_nal_entry* d_index, uint64_t index_cap, uint32_t header_window,
                    hbs_parsed_nal* d_parsed, hbs_slice_compact* d_compact, uint8_t* d_structs, uint64_t structs_cap, uint64_t* d_payload_off,
                    hbs_summary* d_scan_summary, hbs_summary* d_parse_summary, uint64_t* nal_count_out);

/*
 * ---- access units ------------------------------------------------------------------------------------------------
 * hbs_access_units groups the NALs of an indexed and parsed stream into access units (AUs: one coded picture of layer 0
 * with the NALs that belong to it, H.265 7.4.2.4.4) and gives every picture its PicOrderCntVal (8.3.1), on the device.
 * The inputs are what hbs_parse_headers_compact / hbs_parse_materialize / hbs_index_parse_compact wrote, untouched:
 * d_index, d_parsed, d_compact (n_nals records each, 16-byte aligned) and the struct arena d_structs (may be NULL: every
 * SPS then counts as "without a struct").  The fields are taken as the parse writes them (nal_unit_type -1..63, anything
 * else counts as -1; nuh_temporal_id_plus1 0..7); nothing is checked against the stream.  This comment is the specification;
 * tests/_au_ref.py restates it as one loop over the NALs and one over the pictures.
 *
 * Grouping (layer 0 only; NAL types are looked at whatever the layer unless said otherwise).
 *   VCL(k):   nal_unit_type 0..31 and nuh_layer_id 0.
 *   FIRST(k): VCL(k) and d_compact[k].first_slice_segment_in_pic_flag != 0.
 *   CAND(k):  FIRST(k), or nuh_layer_id 0 and type in {32, 33, 34, 35, 39, 41..44, 48..55}.
 *   NAL k starts an AU iff k == 0, or CAND(k) and no CAND NAL lies strictly between the last VCL NAL in front of k and k
 *   (with v(k) / c(k) = the number of the last VCL / CAND NAL < k, -1 for none: CAND(k) && c(k) <= v(k)).  Every other
 *   NAL -- suffix SEI, EOS, filler, NALs of other layers, NALs of type -1, slice segments that continue a picture --
 *   belongs to the AU in progress.  The picture NAL of an AU is its first VCL NAL; an AU without one has
 *   HBS_AU_NO_PICTURE (a batch without any VCL NAL is one such AU).
 *
 * Picture order count, over the pictures (AUs with a picture NAL) in stream order.
 *   Max(p) = 1 << (4 + clamp(v, 0, 12)), v = log2_max_pic_order_cnt_lsb_minus4 of the last SPS NAL (type 33, any layer) in
 *   front of the picture NAL whose struct_off != ~0, read at d_structs + struct_off + hbs_au_sps_poc_offset() (struct_off
 *   is a multiple of 4); none in front in THIS call: v = 0, the parser's all-zero set.  The carry holds no SPS: a batch
 *   that continues another one must begin with (a copy of) the SPS in force if its first pictures are to use it.
 *   A(p) = the nearest picture in front of p with HBS_AU_ANCHOR, else the carry's anchor, else lsb 0, msb 0.
 *   With prev = lsb(A(p)) and lsb = poc_lsb(p) = d_compact[picture NAL].slice_pic_order_cnt_lsb:
 *     d(p) = +Max(p) if lsb < prev && prev - lsb >= Max(p) / 2;  -Max(p) if lsb > prev && lsb - prev > Max(p) / 2;  else 0
 *     msb(p) = 0 if p has HBS_AU_CVS_START, else msb(A(p)) + d(p);   pic_order_cnt = msb(p) + lsb
 *   in 32-bit wrap-around arithmetic.  Out-of-spec input (an IRAP with temporal id > 0, Max changing inside a CVS, any
 *   lsb) has no special case: these formulas are the definition.
 *
 * d_summary: nal_count = AUs, nal_found = n_nals, reserved[0] = pictures, reserved[1] = AUs with HBS_AU_CVS_START,
 * stream_bytes = unit_end of the last AU, rbsp_bytes = 0, stop_reason = 0, error = HBS_E_CAPACITY when au_cap < AUs (then
 * nothing is written to d_au, d_nal_au, d_carry_out; the counts are still right).  d_au == NULL: plan only (the summary
 * alone is written).  n_nals == 0 is valid: no AU, the carry passes through.  n_nals > 2^32 - 1, a missing or misaligned
 * pointer: HBS_E_ARG at once, nothing touched.  `initial` (HOST pointer; NULL: the start of a stream) is the d_carry_out
 * of the batch in front; a continuing batch is expected to begin at an AU boundary (NAL 0 always starts an AU), and with a
 * carry "the first picture of the call" reads "no picture seen yet".  Nothing is stored outside d_au[0, AUs),
 * d_nal_au[0, n_nals), the carry and the summary; no load goes past n_nals records or, in d_structs, outside the word named.
 */
typedef struct hbs_access_unit {      /* 64 bytes */
    uint64_t first_nal;               /* number of the AU's first NAL                                              */
    uint64_t unit_begin;              /* stream offset where that NAL's unit begins: index[first_nal-1].end, 0 for NAL 0
                                         (the filter's definition of a unit)                                       */
    uint64_t unit_end;                /* index[last NAL of the AU].end                                             */
    uint32_t nal_count;               /* NALs in the AU                                                            */
    uint32_t vcl_count;               /* of them VCL NALs (type < 32) with nuh_layer_id 0                          */
    uint32_t first_vcl;               /* the picture NAL: first such VCL NAL, relative to first_nal; ~0u: none     */
    int32_t  nal_unit_type;           /* of the picture NAL (-1: none)                                             */
    int32_t  temporal_id_plus1;       /* of the picture NAL (0: none)                                              */
    int32_t  pic_order_cnt;           /* PicOrderCntVal (8.3.1), two's-complement wrap-around; 0 without a picture */
    int32_t  poc_lsb;                 /* slice_pic_order_cnt_lsb of the picture NAL as the parse reports it        */
    uint32_t slice_types;             /* bit t set: a VCL NAL of the AU with dependent_slice_segment_flag == 0 has
                                         slice_type t (0..2), both as d_compact reports them                       */
    uint32_t flags;                   /* HBS_AU_*                                                                  */
    uint32_t reserved;                /* 0                                                                         */
} hbs_access_unit;

#define HBS_AU_IRAP        1   /* picture NAL type 16..23                                                     */
#define HBS_AU_IDR         2   /* 19, 20                                                                      */
#define HBS_AU_CVS_START   4   /* IRAP with NoRaslOutputFlag = 1: IDR, BLA (16..18), or a CRA / reserved IRAP
                                  (21..23) that is the first picture of the call (no carry) or the first picture
                                  behind an end-of-sequence NAL (type 36)                                     */
#define HBS_AU_ANCHOR      8   /* may serve as prevTid0Pic: temporal_id_plus1 == 1, type not 6..9 (RADL, RASL)
                                  and not a sub-layer non-reference picture (even types 0..14)                */
#define HBS_AU_NO_PICTURE 16   /* no VCL NAL with layer 0                                                     */
#define HBS_AU_DAMAGED    32   /* holds a NAL whose d_parsed rc < 0 and whose type is not one of the types
                                  read_hevc_nal_unit never reads (35..40, 41..47, 48..63), or nal_unit_type -1 */
#define HBS_AU_PARAM_SETS 64   /* holds a VPS, SPS or PPS                                                     */
#define HBS_AU_END_OF_SEQ 128  /* holds an end-of-sequence (36) or end-of-bitstream (37) NAL                  */

typedef struct hbs_au_carry {         /* 16 bytes: the state behind a batch, for the batch that continues it */
    uint32_t flags;                   /* 1: a picture was seen, 2: an anchor exists, 4: an EOS NAL is pending */
    int32_t  anchor_poc_lsb, anchor_poc_msb;
    uint32_t reserved;
} hbs_au_carry;

int hbs_access_units(hbs_ctx* ctx, const hbs_nal_entry* d_index, const hbs_parsed_nal* d_parsed,
                     const hbs_slice_compact* d_compact, const uint8_t* d_structs, uint64_t n_nals,
                     const hbs_au_carry* initial /* HOST pointer, NULL: start of a stream */,
                     hbs_access_unit* d_au, uint64_t au_cap, uint32_t* d_nal_au /* optional: AU number per NAL */,
                     hbs_au_carry* d_carry_out /* optional, device */, hbs_summary* d_summary);
/* Alignment: d_index, d_parsed, d_compact, d_au, d_summary 16 bytes; d_structs, d_nal_au, d_carry_out 4 bytes. */
uint64_t hbs_au_sps_poc_offset(void);   /* offsetof(hevc_sps_t, log2_max_pic_order_cnt_lsb_minus4), like hbs_sps_tables_offset() */

/*
 * From a range of access units to the keep mask of hbs_filter_annexb(..., rule = NULL, d_keep, ...):
 * d_keep[k] = 1 iff first_au <= d_nal_au[k] < first_au + au_count, else 0.  With HBS_AUKEEP_PARAM_SETS additionally 1 for
 * the last VPS (32), the last SPS (33) and the last PPS (34) NAL (any layer), each with d_parsed rc >= 0, in front of the
 * first NAL of AU first_au -- the library's own model of "the sets in force": the last of each kind, ids ignored.  An empty
 * range (au_count 0, or first_au past the last AU) is all zeros, parameter sets included; a range that ends past the last
 * AU is clipped.  d_nal_au is what hbs_access_units wrote for the same n_nals.
 * Alignment: d_nal_au 4 bytes; d_parsed 8 bytes; d_keep any byte.
 */
#define HBS_AUKEEP_PARAM_SETS 1
int hbs_au_keep(hbs_ctx* ctx, const uint32_t* d_nal_au, const hbs_parsed_nal* d_parsed, uint64_t n_nals,
                uint64_t first_au, uint64_t au_count, int flags, uint8_t* d_keep /* n_nals bytes */);

/*
 * ---- decode and presentation times of access units ------------------------------------------------------------------
 * hbs_au_times turns the picture order counts that hbs_access_units wrote into the d_dts / d_pts tables that hbs_ts_mux,
 * hbs_mp4_fragment, hbs_mp4_stbl_write and hbs_rtp_pack read, on the device: a raw Annex-B stream carries no
 * times, and "pts = dts = base_time + a * duration" (what those calls do without tables) is wrong for every stream with
 * reordered pictures.  The AUs of each coded video sequence are ranked by picture order count; an AU is presented in the slot
 * of its rank.  Of d_au[a] only `flags` and `pic_order_cnt` are read; a GOP cut is passed as d_au + first_au.  This comment is
 * the specification; tests/_au_times_ref.py restates it with one sort per segment.  Out-of-spec input has no special case: the
 * formulas are the definition.
 *
 * SEGMENTS.  AU a begins a segment iff a == 0 or d_au[a].flags holds HBS_AU_CVS_START.  s(a) = the first AU of a's segment.
 *
 * KEY.  p(a) = the nearest AU at or in front of a without HBS_AU_NO_PICTURE; key(a) = d_au[p(a)].pic_order_cnt as a signed
 * 32-bit value, -2^31 when the call holds no such AU.  (A segment start other than AU 0 has a picture in every table that
 * hbs_access_units wrote, so p(a) lies in a's segment but for the -2^31 case; a table where it does not is ranked by the same
 * formula.)
 *
 * OUTPUT SLOT.  o(a) = s(a) + #{ b in a's segment : (key(b), b) < (key(a), a) } in lexicographic order: equal keys go in decode
 * order.  o is a permutation of [0, n_aus) that maps every segment onto itself.  Equivalently
 *   o(a) = a + #{ b > a in the segment : key(b) < key(a) } - #{ b < a in the segment : key(b) > key(a) }.
 *
 * SPAN (a stated limit).  back(a) = a - min{ b < a in the segment : key(b) > key(a) } and fwd(a) = max{ b > a in the segment :
 * key(b) < key(a) } - a, each 0 when there is no such b.  An AU with back(a) or fwd(a) above HBS_AUT_MAX_SPAN offends: the
 * summary's error is HBS_E_DEPTH, reserved[0] = 1 + the lowest offending AU, every other count 0, and nothing but the summary
 * is written.  H.265 bounds the number of reordered pictures (15), not their distance, but a B-pyramid of GOP 64 has span 63;
 * the limit bounds the work on any table at 2 * HBS_AUT_MAX_SPAN steps an AU.
 *
 * TIMES.  R = max over a of (a - o(a)), the smallest delay that keeps pts >= dts; 0 <= R <= HBS_AUT_MAX_SPAN.
 *   delay = params->delay with HBS_AUT_DELAY_GIVEN, else R
 *   dts(a) = base_time + a * tick                pts(a) = base_time + (o(a) + delay) * tick
 * both exact, and with HBS_AUT_WRAP33 both then reduced modulo 2^33 (what hbs_ts_mux takes).  With delay >= R, pts(a) >= dts(a)
 * for every AU.  A stream cut into batches (at segment starts) uses one delay for all of them through HBS_AUT_DELAY_GIVEN.
 * d_order[a] = o(a); d_display[o(a)] = a.
 *
 * d_summary on success: nal_count = n_aus, nal_found = segments, rbsp_bytes = the first AU of the last segment (where a caller
 * who works in batches cuts), stream_bytes = 0, stop_reason = 0, reserved[0] = the delay used, reserved[1] = R, reserved[2] =
 * AUs with exact pts < dts (only possible with a given delay < R), error = 0.
 *
 * All four output pointers NULL: plan only, the summary alone is written.  n_aus == 0 is valid: all counts 0, reserved[0] =
 * params->delay when given, else 0.  Refused with HBS_E_ARG at once, nothing touched: unknown flags, non-zero `reserved`,
 * tick == 0, base_time >= 2^62, n_aus > 2^32 - 1, base_time + (n_aus + D) * tick >= 2^62 with D = params->delay when given, else
 * HBS_AUT_MAX_SPAN (this bounds every time on the host: the device has no time error), a missing ctx, params or d_summary, a
 * missing d_au with n_aus > 0, a misaligned pointer.
 * Alignment: d_au, d_summary 16 bytes; d_dts, d_pts 8 bytes; d_order, d_display 4 bytes.
 * Nothing is stored outside the first n_aus entries of the tables given and the summary; no load goes past d_au[n_aus).  No
 * host wait (HIP graphs, above).  Scratch: the context's workspace, sized by n_aus alone -- 17 bytes an AU (key, prefix maximum,
 * suffix minimum and slot, 4 bytes each, and a byte of flags) and 32 bytes per 256 AUs.
 */
#define HBS_AUT_MAX_SPAN     1024u /* stated limit, see SPAN */
#define HBS_AUT_DELAY_GIVEN  1u    /* use params->delay instead of the smallest delay that keeps pts >= dts */
#define HBS_AUT_WRAP33       2u    /* both outputs modulo 2^33 (what hbs_ts_mux takes) */

typedef struct hbs_au_times_params {   /* HOST memory, 32 bytes */
    uint32_t flags;        /* HBS_AUT_* */
    uint32_t tick;         /* duration of one AU in the caller's timescale, >= 1 */
    uint64_t base_time;    /* dts of AU 0, below 2^62 */
    uint32_t delay;        /* with HBS_AUT_DELAY_GIVEN: output slots the presentation lags the decode by */
    uint32_t reserved[3];  /* 0 */
} hbs_au_times_params;

int hbs_au_times(hbs_ctx* ctx, const hbs_access_unit* d_au, uint64_t n_aus,
                 const hbs_au_times_params* params,
                 uint64_t* d_dts, uint64_t* d_pts,        /* optional, each on its own, n_aus */
                 uint32_t* d_order, uint32_t* d_display,  /* optional, each on its own, n_aus */
                 hbs_summary* d_summary);

/*
 * ---- Common Encryption (ISO/IEC 23001-7, scheme `cenc`): subsample table and AES-128-CTR in place -------------------------
 * Two device calls.  hbs_cenc_subsamples writes the subsample table of every sample from tables alone; hbs_cenc_crypt applies
 * AES-128 in counter mode, in place, to the protected ranges of samples that lie anywhere in a buffer.  Encryption and
 * decryption are the same call.  NOT written or read: senc, saiz, saio, sinf / tenc, pssh (the records below are in the senc
 * entry form -- 16-bit clear, 32-bit protected -- so a writer can follow: hbs_mp4_protect and hbs_mp4_init_protect_host, below); the schemes cbcs, cens, cbc1 (params->scheme is there
 * for them; anything but cenc is refused -- cbcs is a call of its own, hbs_cbcs_crypt, below); key rotation (one key a call).
 *
 * hbs_cenc_subsamples.  The samples are exactly those of hbs_mp4_fragment / hbs_annexb_to_lenpref: sample a is the kept NALs
 * k (d_keep NULL: all) with d_nal_au[k] - d_nal_au[0] == a, in index order, each a record of L = params->length_size length
 * bytes and end - start payload bytes; the index and AU-number rules are hbs_mp4_fragment's (start <= end <= stream_bytes,
 * start_k >= end_{k-1}, a kept payload fits L bytes, the AU numbers rise by 0 or 1 and the last is d_nal_au[0] + n_aus - 1).
 * The only stream byte read is the first payload byte b of a kept, non-empty NAL: type = (b >> 1) & 63.
 *   RULE, per sample: C = 0.  For each kept NAL in order, size = end - start:
 *     type >= 32 or size == 0     C += L + size.
 *     type < 32 (a VCL NAL)       its clear lead h = d_payload_off[k] - start with d_payload_off (as hbs_index_parse* wrote it:
 *                                 the stream offset of the first slice data byte), else min(params->clear_lead, size);
 *                                 P = size - h; with HBS_CENC_ALIGN16, P mod 16 bytes move from P to h; C += L + h; if P > 0,
 *                                 emit (C, P) and C = 0.
 *   At the sample's end a remaining C > 0 is emitted as (C, 0).
 *   EMIT (C, P): q = max(ceil(C / 65535), 1) - 1 entries (65535, 0), then (C - 65535 q, P).  (0, P) is one entry; an empty sample
 *   has none.
 * d_sub_first[a] = the entries of all samples below a; d_sub_first[n_aus] = the total.  d_sub[0, total) are the entries.
 * d_summary: nal_count = entries, nal_found = n_nals, rbsp_bytes = protected bytes in all, stream_bytes = sample bytes in all
 * (hbs_mp4_fragment's B(n_aus)), reserved[2] = kept NALs, stop_reason = 0.  error = HBS_E_ARG with reserved[0] = 1 + the lowest
 * offending NAL for a broken index or AU-number rule, or a kept, non-empty VCL NAL whose d_payload_off[k] is ~0, below start + 2
 * or above end (a slice the parse did not read must not silently stay clear); the counts mean nothing then.  Else
 * HBS_E_CAPACITY when, with a d_sub, sub_cap is below the total; the counts are right.  On an error only the summary is
 * written.  d_sub == NULL: plan only -- the summary and d_sub_first are written.  n_nals == 0 with n_aus == 0 is valid.
 * Refused with HBS_E_ARG at once, nothing touched: params NULL, a length_size other than 1, 2, 4, unknown flags, reserved != 0,
 * clear_lead < 2, n_nals or n_aus above 2^32 - 1, n_nals == 0 with n_aus != 0, a missing d_index, d_nal_au or (stream_bytes > 0)
 * d_stream with n_nals > 0, a missing d_sub_first or d_summary, a misaligned pointer.
 * Alignment: d_stream, d_summary 16 bytes; d_index, d_payload_off, d_sub_first, d_sub 8 bytes; d_nal_au 4 bytes; d_keep any.
 * No host synchronisation (HIP graphs, above).  Scratch: the context's workspace, 128 bytes per 2 048 NALs.  The work is
 * parallel over NALs; the clear runs are a segmented scan, the entry numbers a plain one.
 *
 * hbs_cenc_crypt.  Sample s is d_data[off_s, off_s + size_s) with off_s = d_sample_off[s], size_s = d_sample_size[s]: the form
 * hbs_mp4_fragment, hbs_mp4_samples and hbs_mp4_stbl_samples write.  Its subsamples are d_sub[d_sub_first[s], d_sub_first[s+1]),
 * laid end to end from off_s: `clear` bytes untouched, then `protect` bytes.
 *   KEYSTREAM: the protected bytes of a sample, concatenated, are XORed with one continuous keystream: byte j of the
 *   concatenation with byte j mod 16 of AES-128_key(ctr_s + floor(j / 16)).  ctr_s is the sample's 16-byte counter block,
 *   big-endian; the addition touches bytes 8..15 only and wraps from FF..FF to 0 with no carry into bytes 0..7.  A keystream
 *   block may straddle two or more subsamples; no keystream is skipped at a subsample's start.
 *   iv_mode 0: ctr_s = d_iv[16 s, 16 s + 16) (a caller with 8-byte IVs stores the IV followed by eight zero bytes).
 *   iv_mode 1: ctr_s = (the big-endian 64-bit value of iv0[0, 8) + s mod 2^64) followed by eight zero bytes; iv0[8, 16) is
 *   ignored; d_iv, when given, receives the n_samples blocks.
 * CHECKS, each made before any byte of d_data changes: off_s + size_s <= data_bytes without a wrap; off_s + size_s <= off_(s+1)
 * (ascending and disjoint: the call is in place); d_sub_first non-decreasing from 0 (and below 2^48); the entries of sample s add
 * up to exactly size_s; clear <= 65535.  Else error = HBS_E_ARG with reserved[0] = 1 + the lowest offending sample, and nothing
 * but the summary is written.  (The checks run in three groups -- offsets, sizes and d_sub_first; then clear; then the sums -- and
 * the sample named is the lowest of the first group that fails: the entries are not read through a d_sub_first that is wrong.)  d_sub must hold d_sub_first[n_samples] entries: that is the caller's word.
 * d_summary: nal_count = entries read, nal_found = n_samples, rbsp_bytes = bytes XORed, stream_bytes = data_bytes,
 * stop_reason = 0.  n_samples == 0 is valid.
 * Refused with HBS_E_ARG at once, nothing touched: params NULL, a scheme other than HBS_CENC_SCHEME_CENC, iv_mode above 1, flags
 * or reserved != 0, iv_mode 0 without d_iv (n_samples > 0), n_samples above 2^32 - 1, missing tables with n_samples > 0, a
 * missing d_data with data_bytes > 0, a missing d_summary, a misaligned pointer.
 * Alignment: d_data, d_iv, d_summary 16 bytes; d_sample_off, d_sample_size, d_sub_first, d_sub 8 bytes.
 * No byte outside the protected ranges is stored -- not the bytes that share a 16-byte granule with a range's first or last
 * byte either -- beyond d_iv (iv_mode 1) and the summary; no load touches a granule that holds no byte of d_data[0, data_bytes);
 * no host synchronisation.  The key is expanded on the host (176 bytes of round keys) and goes to the kernels by value: it is
 * never stored in the context's scratch or any other device buffer.  Scratch: 16 bytes a sample, 64 per 256 samples, 65 KiB.
 * To DECRYPT fragments that carry their tables in senc boxes, hbs_mp4_senc_samples (below) writes d_sub_first, d_sub and d_iv in
 * the form this call reads with iv_mode 0.
 */
#define HBS_CENC_ALIGN16      1u            /* hbs_cenc_plan_params.flags: protected ranges are whole 16-byte blocks */
#define HBS_CENC_SCHEME_CENC  0x63656E63u   /* 'cenc' */

typedef struct hbs_cenc_subsample { uint32_t clear /* <= 65535 */, protect; } hbs_cenc_subsample;   /* 8 bytes */

typedef struct hbs_cenc_plan_params {   /* HOST memory, 16 bytes */
    int32_t  length_size;   /* 1, 2, 4: as hbs_annexb_to_lenpref */
    uint32_t flags;         /* HBS_CENC_ALIGN16 */
    uint32_t clear_lead;    /* with d_payload_off == NULL: payload bytes of a VCL NAL that stay clear (>= 2) */
    uint32_t reserved;      /* 0 */
} hbs_cenc_plan_params;

typedef struct hbs_cenc_params {        /* HOST memory, 48 bytes */
    uint8_t  key[16];
    uint8_t  iv0[16];       /* iv_mode 1 */
    uint32_t scheme;        /* HBS_CENC_SCHEME_CENC; anything else: HBS_E_ARG */
    uint32_t iv_mode;       /* 0: d_iv is read; 1: sequential, d_iv (nullable) is written */
    uint32_t flags, reserved;   /* 0 */
} hbs_cenc_params;

int hbs_cenc_subsamples(hbs_ctx* ctx, const uint8_t* d_stream, uint64_t stream_bytes,
                        const hbs_nal_entry* d_index, uint64_t n_nals, const uint8_t* d_keep /* nullable */,
                        const uint32_t* d_nal_au, uint64_t n_aus,
                        const uint64_t* d_payload_off /* nullable: as hbs_index_parse* wrote it */,
                        const hbs_cenc_plan_params* params,
                        uint64_t* d_sub_first /* n_aus + 1 */, hbs_cenc_subsample* d_sub /* NULL: plan only */, uint64_t sub_cap,
                        hbs_summary* d_summary);
int hbs_cenc_crypt(hbs_ctx* ctx, uint8_t* d_data, uint64_t data_bytes,
                   const uint64_t* d_sample_off, const uint64_t* d_sample_size, uint64_t n_samples,
                   const uint64_t* d_sub_first /* n_samples + 1 */, const hbs_cenc_subsample* d_sub,
                   uint8_t* d_iv /* n_samples x 16 bytes */, const hbs_cenc_params* params, hbs_summary* d_summary);

/*
 * ---- Common Encryption, scheme `cbcs` (ISO/IEC 23001-7 10.4): AES-128-CBC over a pattern of blocks, in place ------------------
 * hbs_cbcs_crypt is the call for the scheme that HLS / FairPlay and CMAF ask for: of every protected range, crypt_byte_block
 * 16-byte blocks are enciphered in CBC mode, skip_byte_block blocks stay clear, and so on (video: 1 and 9).  It takes the tables
 * of hbs_cenc_crypt, above -- the subsample table of hbs_cenc_subsamples is the same for every scheme -- and a params record of
 * its own.  CBC is not its own inverse: HBS_CBCS_DECRYPT selects the way back.  NOT done: cens and cbc1; senc, saiz, saio,
 * sinf / tenc, pssh (hbs_mp4_protect and hbs_mp4_init_protect_host, below, write them); key rotation (one key a call).
 *
 * Sample s is d_data[off_s, off_s + size_s) with off_s = d_sample_off[s], size_s = d_sample_size[s]; its subsamples are
 * d_sub[d_sub_first[s], d_sub_first[s+1]), laid end to end from off_s: `clear` bytes untouched, then `protect` bytes.
 *   RULE, per entry (clear, protect) whose protected range begins at address p, with c = crypt_byte_block and
 *   k = skip_byte_block (c = k = 0 means c = 1, k = 0: every block):
 *     nb = floor(protect / 16); block i < nb is d_data[p + 16 i, p + 16 i + 16), r = i mod (c + k).
 *     Block i is a CRYPT BLOCK iff r < c -- and, with HBS_CBCS_WHOLE_RUNS, i - r + c <= nb as well: a last run of fewer than c
 *     whole blocks stays clear.  With f = floor(nb / (c + k)) and m = nb mod (c + k) an entry has f c + min(m, c) crypt blocks
 *     without the flag and f c + (m >= c ? c : 0) with it; the j-th of them is block floor(j / c) (c + k) + j mod c.
 *     The crypt blocks of ONE entry, in order, are one CBC chain that starts from the sample's IV:
 *       encrypt   C_j = AES-128_key(P_j xor C_(j-1)),       C_(-1) = IV_s
 *       decrypt   P_j = AES-128^-1_key(C_j) xor C_(j-1)
 *     Chain and pattern restart at every entry: two entries of one sample with equal plaintext give equal ciphertext.
 *     Every other byte is neither changed nor stored: skip blocks, the protect mod 16 bytes behind the last whole block, clear
 *     bytes, the gaps between samples, and the bytes that share a 16-byte granule of memory with a crypt block (p is any
 *     address).
 *   The two readings of a truncated last run -- partly enciphered, or left clear -- exist in the field; they differ only for
 *   c > 1.  1:9 and 1:0 (and 0:0) give the same bytes under both, and HBS_CBCS_WHOLE_RUNS selects between them otherwise.
 *   iv_mode 0: IV_s = d_iv[16 s, 16 s + 16).  iv_mode 1: IV_s = params->iv0 for every sample (tenc's default_constant_IV, the
 *   usual form of cbcs); d_iv is not read and may be NULL.
 * CHECKS, each made before any byte of d_data changes: exactly those of hbs_cenc_crypt, in its three groups and with its
 * words -- off_s + size_s <= data_bytes without a wrap; off_s + size_s <= off_(s+1); d_sub_first non-decreasing from 0 (and below
 * 2^48); then clear <= 65535; then the entries of sample s add up to exactly size_s.  Else error = HBS_E_ARG with reserved[0] =
 * 1 + the lowest offending sample (of the first group that fails), and nothing but the summary is written.  A protect that is
 * no multiple of 16 is no error (no HBS_CENC_ALIGN16 is needed).  d_sub must hold d_sub_first[n_samples] entries.
 * d_summary: nal_count = entries read, nal_found = n_samples, rbsp_bytes = 16 x the crypt blocks of all entries, stream_bytes =
 * data_bytes, stop_reason = 0, reserved = 0.  n_samples == 0 is valid.
 * Refused with HBS_E_ARG at once, nothing touched: params NULL, iv_mode above 1, unknown flags, crypt_byte_block or
 * skip_byte_block above 15, crypt_byte_block == 0 with skip_byte_block != 0, a reserved field != 0, iv_mode 0 without d_iv
 * (n_samples > 0), n_samples above 2^32 - 1, missing tables with n_samples > 0, a missing d_data with data_bytes > 0, a missing
 * d_summary, a misaligned pointer.
 * Alignment: d_data, d_iv, d_summary 16 bytes; d_sample_off, d_sample_size, d_sub_first, d_sub 8 bytes.
 * No host synchronisation (HIP graphs, above: a replay uses the key, iv0, direction and pattern of the capture).  Both key
 * schedules -- the cipher's and that of the equivalent inverse cipher -- are expanded on the host and go to the kernel by value
 * with the launch; they are never in the context's scratch or any other device buffer, and the host copies are zeroed when the
 * call returns.  Scratch: that of hbs_cenc_crypt, which the two calls share (16 bytes a sample, 64 per 256 samples, 65 KiB; it
 * is sized without the entry count, which the host never learns).
 * Work: the entries are walked in 1 024 equal ranges, a workgroup a range, 256 entries a step.  An entry of fewer than 64
 * crypt blocks is one lane's serial loop in either direction.  A longer one is, when DECRYPTING, a wavefront's: 64 consecutive
 * crypt blocks a step, each lane's previous ciphertext block taken from the lane below.  When ENCRYPTING it stays on its one
 * lane, because C_j needs C_(j-1): that is CBC, not this library.  A sample of one 1 MiB NAL at 1:9 is about 6 500 dependent
 * blocks on one lane; throughput of encryption comes from many entries, not from long ones.
 * To decrypt protected fragments: hbs_mp4_senc_samples (below) gives d_sub_first, d_sub and, with per-sample IVs, d_iv;
 * hbs_mp4_init_unprotect_host gives the pattern and, with iv_size 0, the constant IV that goes into iv0.
 */
#define HBS_CBCS_DECRYPT     1u   /* flags: the inverse direction (CBC is not its own inverse) */
#define HBS_CBCS_WHOLE_RUNS  2u   /* flags: a last run of fewer than crypt_byte_block whole blocks stays clear */

typedef struct hbs_cbcs_params {      /* HOST memory, 48 bytes */
    uint8_t  key[16];
    uint8_t  iv0[16];                 /* iv_mode 1: the constant IV of every sample (tenc default_constant_IV) */
    uint32_t iv_mode;                 /* 0: d_iv[16 s, 16 s + 16) is sample s's IV; 1: iv0 for every sample, d_iv not read */
    uint32_t flags;                   /* HBS_CBCS_DECRYPT | HBS_CBCS_WHOLE_RUNS */
    uint8_t  crypt_byte_block;        /* 0..15, as in tenc; video: 1 */
    uint8_t  skip_byte_block;         /* 0..15; video: 9 */
    uint16_t reserved0;               /* 0 */
    uint32_t reserved1;               /* 0 */
} hbs_cbcs_params;

int hbs_cbcs_crypt(hbs_ctx* ctx, uint8_t* d_data, uint64_t data_bytes,
                   const uint64_t* d_sample_off, const uint64_t* d_sample_size, uint64_t n_samples,
                   const uint64_t* d_sub_first /* n_samples + 1 */, const hbs_cenc_subsample* d_sub,
                   const uint8_t* d_iv /* n_samples x 16 bytes, iv_mode 0 */,
                   const hbs_cbcs_params* params, hbs_summary* d_summary);

/*
 * ---- protected fragments: saiz, saio and senc into every traf on the device; encv / sinf / tenc and pssh on the host -------
 * hbs_mp4_protect is the writer the records above were laid out for.  It puts the sample auxiliary information -- which IV
 * each sample has, where its clear and protected ranges lie -- into the fragments hbs_mp4_fragment wrote, and fixes the sizes
 * and the trun's data offset; hbs_mp4_init_protect_host makes the init segment say that the track is protected.  With them
 * fragment -> hbs_cenc_subsamples -> protect -> crypt yields segments a cenc / cbcs player can decrypt.  Every integer in a box
 * is big-endian.  tests/_mp4_protect_ref.py restates the rule as one loop.
 *
 * INPUT.  Fragment r is d_in[out_off_r, out_off_r + out_bytes_r) of d_frag[r]: the table hbs_mp4_fragment wrote (hbs_mp4_samples
 * writes the same form).  Fragments may lie anywhere in d_in, in any order, with anything between them.  Sample numbering is
 * the pointer-offset rule of the other calls: first_au_r - first_au_0 equals the sum of `samples` of the fragments below r,
 * and the total is n_samples.  Sample s of the call has the entries d_sub[d_sub_first[s], d_sub_first[s+1]) and the IV
 * d_iv[16 s, 16 s + iv_size): the table hbs_cenc_crypt reads, or writes with iv_mode 1.  d_out must not overlap d_in.
 * FRAGMENT RULE, checked on the device before anything is written.  A fragment is accepted only in the form hbs_mp4_fragment
 * states, with S = samples_r: out_off + out_bytes <= in_bytes without a wrap; out_bytes >= 96 + 16 S; word 0 is 88 + 16 S, then
 * 'moof'; 'traf' at +28 with size 64 + 16 S; 'tfhd' at +36, 'tfdt' at +52; 'trun' at +72 with size 20 + 16 S, version and flags
 * 01 00 0F 01, count S, data_offset 96 + 16 S; at 88 + 16 S an 'mdat' whose size is out_bytes - 88 - 16 S (so that has 32 bits,
 * and S is (2^32 - 89) / 16 at most).  The mfhd, the sequence, the track id and the decode time are not constrained.
 * Anything else, or a broken numbering rule -- fragment r breaks it when first_au_r - first_au_0 is not the sum below r, when
 * that sum + S passes n_samples, or, the last fragment, when it is not n_samples -- is a FRAGMENT ERROR: HBS_E_ARG,
 * reserved[1] = 1 + the lowest such fragment.
 * SAMPLE RULE, with V = iv_size and n_s the entries of sample s; only looked at when no fragment offends.  In two groups, and
 * the sample named is the lowest of the first group that fails (the entries are not read through a d_sub_first that is
 * wrong: hbs_cenc_crypt's way).  First: d_sub_first starts at 0, never decreases and stays below 2^48; n_s <=
 * floor((253 - V) / 6), so that the saiz byte V + 2 + 6 n_s fits; with V == 8 the bytes d_iv[16 s + 8, 16 s + 16) are zero
 * (else the 8-byte IV in the box is not the counter block the sample was enciphered with).  Second: every clear <= 65535; the
 * entries add up to exactly the size word of the sample's trun entry.  A SAMPLE ERROR is HBS_E_ARG, reserved[0] = 1 + that
 * sample.  Behind both: a new moof size above 2^31 - 9 (the trun's data_offset is a signed 32-bit field) is a fragment error.
 * OUTPUT.  The fragments back to back in order; gaps of the input are dropped.  Fragment r, with E entries over its samples:
 *   moof  size M' = 141 + (19 + V) S + 6 E
 *     mfhd  copied
 *     traf  size M' - 24
 *       tfhd, tfdt  copied
 *       trun  copied, but data_offset = M' + 8
 *       saiz  size 17 + S   'saiz' 00 00 00 00  default_sample_info_size 00  sample_count(4) = S, then a byte a sample: V + 2 + 6 n_s
 *       saio  00 00 00 14   'saio' 00 00 00 00  entry_count(4) = 1  offset(4) = 141 + 17 S      (from the moof's first byte)
 *       senc  size 16 + (V + 2) S + 6 E   'senc' 00 00 00 02  sample_count(4) = S,
 *             then a sample: IV (V bytes)  subsample_count(2) = n_s, then n_s x ( clear(2) protect(4) )
 *   mdat  copied whole (header and payload)
 * The fragment grows by 53 + (V + 3) S + 6 E bytes (hbs_mp4_protect_bytes_host); the output is the sum of out_bytes_r plus
 * 53 n_frags + (V + 3) n_samples + 6 E_total.  d_sample_off / d_sample_size (optional, both or neither, n_samples each) give
 * every sample's place in d_out -- its mdat payload offset is the sizes of the trun entries in front of it -- in the form
 * hbs_cenc_crypt, hbs_cbcs_crypt and hbs_lenpref_to_annexb read: enciphering may run before this call on d_in or after it on
 * d_out, with the same bytes either way.  d_frag_out[r] (optional, n_frags) is d_frag[r] with the new out_off and out_bytes.
 *
 * d_summary: nal_count = fragments, nal_found = n_samples, rbsp_bytes = entries in all, stream_bytes = output bytes,
 * stop_reason = 0 (with HBS_E_ARG the two byte counts are 0).  HBS_E_CAPACITY when out_cap is below the output; the counts are
 * right then.  Also HBS_E_CAPACITY, with or without a d_out and with both byte counts 0, when the sum of floor(out_bytes_r /
 * 2^20) plus n_frags reaches 2^41: the output could pass 2^61 bytes.  On any error nothing but the summary is written.
 * d_out == NULL: plan only, the summary alone is written.  n_frags == 0 with n_samples == 0 is valid.
 * Refused with HBS_E_ARG at once, before anything is written: params NULL, an iv_size other than 0, 8, 16, flags or reserved
 * words not 0, iv_size > 0 without a d_iv when n_samples > 0, n_frags or n_samples above 2^32 - 1, n_frags == 0 with n_samples
 * != 0, one of the two sample tables without the other, out_cap above 2^46 with a d_out, a missing d_frag or (in_bytes > 0)
 * d_in with n_frags > 0, a missing d_sub_first or d_sub with n_samples > 0, a missing d_summary, a misaligned pointer.
 * Alignment: d_in, d_out, d_frag, d_frag_out, d_iv, d_summary 16 bytes; d_sub_first, d_sub, d_sample_off, d_sample_size 8.
 * Nothing outside [d_out, d_out + output bytes), d_sample_off / d_sample_size[0, n_samples), d_frag_out[0, n_frags) and the
 * summary is stored; no load touches a 16-byte granule that holds no byte of d_in[0, in_bytes); no host synchronisation (HIP
 * graphs, above).  Scratch comes from the context's workspace and is sized by n_frags, n_samples and out_cap alone: 32 bytes a
 * fragment and 80 per 256 fragments, 80 bytes per 256 samples, 8 bytes per 64 KiB of out_cap with a d_out (so pass what the
 * plan gave as out_cap), every table rounded up to 256 bytes, and 64 bytes.
 *
 * hbs_mp4_init_protect_host (plain C, no GPU).  It walks init[0, n) by the box rule of hbs_mp4_init_read_host to the first
 * 'hvc1' / 'hev1' entry that has an hvcC of the track (track_id 0: as there).  The output is the segment with that entry renamed
 * 'encv', with a sinf appended to the entry -- frma (12 bytes, the original fourcc); schm (20 bytes: version and flags 0, the
 * scheme, version 00 01 00 00); schi holding a tenc: version 0, or 1 when crypt_byte_block or skip_byte_block is not 0; flags 0;
 * 00; crypt_byte_block << 4 | skip_byte_block (00 at version 0); 01; iv_size; the KID; and, with iv_size 0, constant_iv_size
 * and that many bytes of constant_iv -- with the sinf's size added to the 32-bit sizes of the entry, stsd, stbl, minf, mdia,
 * trak and moov, and with the pssh boxes appended at the end of the moov (their bytes added to its size).  Each pssh[i] must be
 * one box of type 'pssh' whose size field equals pssh_bytes[i].  Returns the bytes the segment takes; it is written to out only
 * when cap suffices.  HBS_E_ARG: anything hbs_mp4_init_read_host's walk calls malformed, no such track or entry; one of the seven
 * boxes with a 64-bit size or a size field of 0; a size that would pass 2^32 - 1; a scheme other than 'cenc' and 'cbcs'; a
 * block count above 15; a pattern with 'cenc'; an iv_size other than 0, 8, 16; constant_iv_size other than 8 or 16 with iv_size
 * 0, or other than 0 without; a reserved word not 0; a NULL pointer.  Every length is bounded before it is used; no byte at or
 * behind init + n, or outside the pssh boxes, is read.
 * OUT OF SCOPE: reading senc / encv back (hbs_mp4_samples and hbs_mp4_init_read_host stay as they are: an 'encv' entry is not
 * a video entry to them); key rotation (sbgp / sgpd 'seig'); cens and cbc1; several tracks; building pssh payloads.
 * (Reading back is the business of calls of its own: hbs_mp4_senc_samples and hbs_mp4_init_unprotect_host, below.)
 */
typedef struct hbs_mp4_protect_params {   /* HOST memory, 32 bytes */
    uint32_t iv_size;        /* 0, 8 or 16: IV bytes a sample in the senc; 0: none (tenc's constant IV, the usual cbcs form) */
    uint32_t flags;          /* none defined: 0 */
    uint32_t reserved[6];    /* 0 */
} hbs_mp4_protect_params;

int hbs_mp4_protect(hbs_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes,
                    const hbs_mp4_frag* d_frag, uint64_t n_frags,
                    const uint64_t* d_sub_first /* n_samples + 1 */, const hbs_cenc_subsample* d_sub,
                    const uint8_t* d_iv /* n_samples x 16; read when iv_size > 0 */, uint64_t n_samples,
                    const hbs_mp4_protect_params* params,
                    uint8_t* d_out, uint64_t out_cap,                 /* d_out NULL: plan only */
                    uint64_t* d_sample_off, uint64_t* d_sample_size,  /* optional, both or neither, n_samples: in d_out */
                    hbs_mp4_frag* d_frag_out /* optional, n_frags */,
                    hbs_summary* d_summary);
uint64_t hbs_mp4_protect_bytes_host(uint64_t samples, uint64_t entries, uint32_t iv_size);   /* 53 + (iv_size + 3) S + 6 E */

typedef struct hbs_mp4_tenc {            /* 64 bytes */
    uint32_t scheme;                     /* 'cenc' (0x63656E63) or 'cbcs' (0x63626373) */
    uint8_t  crypt_byte_block, skip_byte_block;   /* 0..15; both 0: tenc version 0 */
    uint8_t  iv_size;                    /* 0, 8, 16: default_Per_Sample_IV_Size */
    uint8_t  constant_iv_size;           /* 8 or 16 with iv_size 0, else 0 */
    uint8_t  kid[16], constant_iv[16];
    uint32_t reserved[6];                /* 0 */
} hbs_mp4_tenc;
int64_t hbs_mp4_init_protect_host(const uint8_t* init, uint64_t n, uint32_t track_id /* 0: as hbs_mp4_init_read_host */,
                                  const hbs_mp4_tenc* t,
                                  const uint8_t* const* pssh, const uint64_t* pssh_bytes, uint64_t n_pssh /* whole 'pssh' boxes */,
                                  uint8_t* out, uint64_t cap);   /* bytes needed; written only when cap suffices; HBS_E_ARG */

/*
 * ---- protected fragments read back: senc to the subsample table and the IVs on the device; encv back to hvc1 on the host ----
 * hbs_mp4_senc_samples is the inverse of hbs_mp4_protect, and reads other packagers' fragments too: from the senc box of every
 * fragment it makes d_sub_first / d_sub / d_iv, the tables hbs_cenc_crypt (iv_mode 0) and hbs_cbcs_crypt read.  With it a
 * protected segment goes hbs_mp4_samples -> hbs_mp4_senc_samples -> hbs_cenc_crypt / hbs_cbcs_crypt(HBS_CBCS_DECRYPT) ->
 * hbs_lenpref_to_annexb and comes out as Annex-B with no byte visiting the host.  tests/_mp4_senc_ref.py restates both calls as
 * one loop each.
 *
 * INPUT.  Fragment r has its moof at d_in + out_off_r and is d_in[out_off_r, out_off_r + out_bytes_r) of d_frag[r]: the table
 * hbs_mp4_samples writes (out_bytes reaches to the next moof) or hbs_mp4_protect's d_frag_out.  Fragments may lie anywhere in
 * d_in, in any order.  Sample numbering is hbs_mp4_protect's pointer-offset rule: first_au_r - first_au_0 equals the sum of
 * `samples` of the fragments below r, and the last sum is n_samples.  A fragment with samples == 0 has only its bounds checked.
 * d_sample_size (optional) is the table hbs_mp4_samples wrote for the same fragments.
 * INSIDE THE MOOF the box rule of hbs_mp4_samples applies: a size of 1 is followed by a 64-bit size, a size of 0 runs to the
 * container's end (the fragment's, for the moof), children of unknown type are stepped over.  Word 1 of the fragment must be
 * 'moof'.  The traf is chosen exactly as hbs_mp4_samples chooses it: the first whose tfhd carries params->track_id (0: the
 * first traf); every traf in front of it must have a well-formed tfhd; every child of the moof and of those trafs must hold
 * the box rule.  tfdt, trun and mfhd are not looked at: `samples` is the caller's word, as hbs_mp4_samples counted it.  Of the
 * chosen traf's children the first 'senc' is read.  Its payload is version/flags(4) sample_count(4), then a sample: IV (V =
 * iv_size bytes) and, with flag 0x2, subsample_count(2) and that many clear(2) protect(4), all big-endian; without flag 0x2
 * nothing more, and the sample is one entry (0, size_s) when size_s > 0 and none otherwise, which needs d_sample_size.  Bytes of
 * the box behind the last sample are ignored.  No mdat byte is ever read.
 * RESULT.  d_sub_first[s] = the entries of the samples below s (n_samples + 1 words, the total last); d_sub the entries in
 * the host byte order of hbs_cenc_subsample; d_iv[16 s, 16 s + 16) the IV: V = 8 the IV and eight zero bytes (the form
 * hbs_cenc_crypt iv_mode 0 reads), V = 16 as stored, V = 0 d_iv is untouched.  On the output of hbs_mp4_protect the three tables
 * are the ones that went into it, value for value.
 * HBS_SENC_CLEAR_IF_ABSENT: a chosen traf without a senc gives each of its samples of size z > 0 the entries of
 * hbs_cenc_subsamples' EMIT(z, 0): ceil(z / 65535) - 1 entries (65535, 0), then the rest; its d_iv is zero; d_sample_size is
 * needed.  Without the flag such a traf is a fragment error.
 * ERRORS, in the two levels of hbs_mp4_protect.  A FRAGMENT ERROR is HBS_E_ARG with reserved[1] = 1 + the lowest fragment for
 * which any of these holds: it leaves the buffer; word 1 is not 'moof', or the moof is larger than out_bytes; a child breaks
 * the box rule; a tfhd is missing or too short; no traf is chosen although samples > 0; the senc's version is not 0 or its
 * flags are other than 0 or 2; its sample_count is not samples_r; a sample of the senc leaves the box; there is no senc and the
 * flag is not set; d_sample_size is missing where the rule needs it; the numbering rule is broken (as hbs_mp4_protect states
 * it).  Only when no fragment offends a SAMPLE ERROR is raised: HBS_E_ARG with reserved[0] = 1 + the lowest sample whose size
 * is above 2^32 - 1 where the size becomes an entry.  A total of entries at or above 2^48 is HBS_E_CAPACITY with zero counts.
 * With a d_sub, sub_cap below the total is HBS_E_CAPACITY with the counts right.  On any error only the summary is written.
 * d_sub == NULL: plan only, the summary and d_sub_first (and d_iv) are written, as hbs_cenc_subsamples does.
 * d_summary: nal_count = entries, nal_found = n_samples, rbsp_bytes = the sum of protect over all entries, stream_bytes =
 * in_bytes, stop_reason = 0, reserved[2] = fragments whose senc was read; with HBS_E_ARG, and at 2^48 entries, nal_count,
 * rbsp_bytes and reserved[2] are 0.
 * Refused with HBS_E_ARG at once, nothing touched: params NULL, an iv_size other than 0, 8, 16, unknown flags, a reserved word
 * not 0, n_frags or n_samples above 2^32 - 1, in_bytes above 2^62, n_frags == 0 with n_samples != 0, a missing d_sub_first or
 * d_summary, a missing d_frag or (in_bytes > 0) d_in with n_frags > 0, iv_size > 0 without a d_iv when n_samples > 0, a
 * misaligned pointer.  Alignment: d_in, d_frag, d_iv, d_summary 16 bytes; d_sample_size, d_sub_first, d_sub 8.
 * No load touches a 16-byte granule that holds no byte of d_in[0, in_bytes); nothing is stored outside d_sub_first[0,
 * n_samples], d_sub[0, total), d_iv[0, 16 n_samples) and the summary; no host synchronisation (HIP graphs, above).  Scratch is
 * a slot of its own in the context's workspace, sized by n_frags and n_samples alone: 64 bytes; 52 bytes a fragment and 80
 * per 256 fragments; 16 bytes a sample, 128 per 256 samples and 64 for each of the min(2 048, 4 per 256 samples) workgroups
 * that write entries; every table rounded up to 256 bytes.
 * WORK.  One lane finds a fragment's boxes.  A lane per sample then takes the traf's saiz as a HINT: the sizes in front of a
 * sample give the place its record would have, the lane reads subsample_count there and accepts the place when V + 2 + 6 n
 * is the hinted size and the record stays in the box.  When every sample of a fragment passes, the places are the serial
 * walk's by induction from sample 0.  A fragment without a usable saiz (none, another sample_count, too short), or with one
 * failed check, is walked by one lane, a step a sample; only that walk can find that a sample leaves the box.  The saiz is
 * never an authority: the result is defined by the senc alone.  The entries are written a lane an entry.
 * STATED LIMITS: PIFF 'uuid' sample encryption boxes; auxiliary information outside a senc (a traf with saio but no senc);
 * key rotation (sbgp / sgpd 'seig'); several tracks in one call; cens / cbc1.
 *
 * hbs_mp4_init_unprotect_host (plain C, no GPU): the inverse of hbs_mp4_init_protect_host.  It walks init[0, n) to the moov
 * (the first; the top-level boxes in front of it hold the box rule of hbs_mp4_init_read_host) and through its children, which
 * all hold it.  A trak with a 32-bit size field is looked at until one is found: its tkhd must be what hbs_mp4_init_read_host
 * accepts; with track_id 0 or the tkhd's id, the first mdia, in it the first minf, stbl and stsd are taken, and of the stsd's
 * entries the first 'encv' that satisfies all of: it holds an hvcC; it holds a sinf (the first) whose frma is 'hvc1' or 'hev1',
 * whose schm is 'cenc' or 'cbcs' and whose schi / tenc has version 0 or 1, isProtected 1, an iv_size of 0, 8 or 16 and, with
 * iv_size 0, a constant IV of 8 or 16 bytes; the record is one hbs_mp4_init_protect_host takes (no pattern with 'cenc').
 * t_out is that record (at tenc version 0 the pattern is 0 whatever the byte holds); it feeds hbs_mp4_senc_params.iv_size and
 * hbs_cbcs_params (crypt_byte_block, skip_byte_block, iv0).  format_out (optional) is the frma fourcc.  pssh_off / pssh_bytes
 * list every 'pssh' that is a direct child of the moov, whole boxes as offsets into init; only the first pssh_cap are
 * written, *n_pssh_out (optional) always is their number.  The output is the segment with that entry renamed to the frma
 * fourcc, that sinf and the pssh boxes removed and the 32-bit sizes of entry, stsd, stbl, minf, mdia, trak and moov reduced;
 * it must be one hbs_mp4_init_read_host accepts for that track with that entry, else HBS_E_ARG.  On the output of
 * hbs_mp4_init_protect_host it returns the segment that went in, byte for byte, and the record that went in.  Returns the
 * bytes the clear segment takes; out is written only when cap suffices; on an error nothing is written.  HBS_E_ARG: anything
 * malformed on the way, no such track or entry, one of the seven boxes with a 64-bit or zero size field, n above 2^62, a NULL
 * init or t_out, a NULL out with cap > 0, NULL lists with pssh_cap > 0.  Every length is bounded before it is used; no byte at
 * or behind init + n is read.
 */
#define HBS_SENC_CLEAR_IF_ABSENT 1u   /* a traf without a senc: its samples are wholly clear (needs d_sample_size) */
typedef struct hbs_mp4_senc_params {  /* HOST memory, 32 bytes */
    uint32_t iv_size;      /* 0, 8, 16: tenc default_Per_Sample_IV_Size */
    uint32_t track_id;     /* as hbs_mp4_read_params.track_id; 0: the first traf */
    uint32_t flags;        /* HBS_SENC_CLEAR_IF_ABSENT */
    uint32_t reserved[5];  /* 0 */
} hbs_mp4_senc_params;

int hbs_mp4_senc_samples(hbs_ctx* ctx, const uint8_t* d_in, uint64_t in_bytes,
                         const hbs_mp4_frag* d_frag, uint64_t n_frags,          /* as hbs_mp4_samples / hbs_mp4_protect wrote it */
                         const uint64_t* d_sample_size /* nullable, n_samples: as hbs_mp4_samples wrote it */, uint64_t n_samples,
                         const hbs_mp4_senc_params* params,
                         uint64_t* d_sub_first /* n_samples + 1 */, hbs_cenc_subsample* d_sub /* NULL: plan only */, uint64_t sub_cap,
                         uint8_t* d_iv /* n_samples x 16; written when iv_size > 0; nullable when 0 */,
                         hbs_summary* d_summary);
int64_t hbs_mp4_init_unprotect_host(const uint8_t* init, uint64_t n, uint32_t track_id /* 0: the first track with such an entry */,
                                    hbs_mp4_tenc* t_out, uint32_t* format_out /* frma: 'hvc1' / 'hev1' */,
                                    uint64_t* pssh_off, uint64_t* pssh_bytes, uint64_t pssh_cap, uint64_t* n_pssh_out,
                                    uint8_t* out, uint64_t cap);   /* bytes the clear init segment takes; written only when cap suffices */

/*
 * ---- access-unit delimiters and parameter sets in front of access units ---------------------------------------------
 * hbs_au_insert makes an elementary stream fit for the container or segment it goes into: an access-unit delimiter (AUD, type
 * 35; 13818-1 wants one per HEVC AU in a transport stream) in front of every picture that has none, and a copy of the
 * parameter sets in force in front of every IRAP picture (and, when asked, of the first AU), so that every segment cut at an
 * IRAP decodes alone.  Pure byte movement on the device over what the library already holds: the stream, d_index / d_parsed
 * (n_nals records each) and what hbs_access_units wrote for them over the whole batch, d_au (n_aus records) and d_nal_au.  It
 * also produces the output's index, AU table and per-NAL AU numbers, so hbs_ts_mux and hbs_annexb_to_lenpref run on the
 * result without a second scan or parse.  This comment is the specification; tests/_auins_ref.py restates it as one loop over
 * the AUs.
 *
 * THE RANGE.  AUs [first_au, first_au + au_count), clipped as hbs_au_keep clips it: empty when au_count is 0 or first_au is
 * past the last AU, cut at n_aus otherwise.  An empty range gives an empty output.  NAL types and rc are taken from d_parsed
 * as the parse wrote them (as hbs_au_keep takes them); nothing is read from the stream to classify.
 *
 * AU a OF THE RANGE.  f = first_nal, p = f + first_vcl, or f + nal_count when first_vcl == ~0u.
 *   Insertion point   I = d_index[f].end if d_parsed[f].nal_unit_type == 35 (the AU begins with an AUD of its own: what is
 *                     inserted goes behind it), else I = unit_begin.
 *   AUD               inserted at I iff HBS_AUINS_AUD is set, the AU has no HBS_AU_NO_PICTURE and d_parsed[f].nal_unit_type
 *                     != 35.  It is the seven bytes 00 00 00 01 46 T X: T = temporal_id_plus1 & 7 of the AU record,
 *                     X = pic_type << 5 | 0x10 with pic_type 0 when slice_types == 4 (I only), 1 when slice_types != 0,
 *                     != 4 and bit 0 is clear (P and I), else 2 (which includes slice_types == 0).  No special case for
 *                     out-of-spec values: the formula is the definition.  hbs_aud_nal_host writes the same bytes.
 *   Parameter sets    considered iff HBS_AUINS_PARAM_SETS is set and the AU has HBS_AU_IRAP, or HBS_AUINS_PARAM_SETS_FIRST is
 *                     set and a is the first AU of the clipped range.  For each kind t = 32, 33, 34 in that order, q_t = the
 *                     last NAL k < p with nal_unit_type == t and rc >= 0, of any layer and id, over the whole batch (the
 *                     library's model of "the sets in force", as hbs_au_keep's).  No such NAL, or q_t >= f (the AU brings
 *                     its own): nothing for t.  Otherwise 00 00 00 01 and stream[start_q, end_q) are inserted, behind the
 *                     inserted AUD if there is one, else at I.
 *   Output bytes      for every AU of the range in order: stream[unit_begin, I), the insertions, stream[I, unit_end).  An
 *                     AU without insertions is copied verbatim.
 *                     A copied set keeps its nuh_layer_id: one of another layer begins no access unit (7.4.2.4.4), so in
 *                     front of an AU without an AUD a regrouping of the output counts it to the AU in front; d_au_out
 *                     counts it to the AU it was inserted into.
 *
 * OUTPUT TABLES, all optional, all relative to the output, which has M NALs (index_cap: the room each of the three per-NAL
 * tables has, in entries; d_au_out has room for the clipped range).
 *   d_index_out[j]    start / end: the payload in the output.  rbsp_len 3 for an inserted AUD, the source entry's otherwise;
 *                     rbsp_off the running sum of rbsp_len.  status 0 for an inserted AUD, else the source status with
 *                     HBS_ST_UNTERMINATED cleared and then set on the last output entry only (the filter's rule).
 *   d_nal_src[j]      the source NAL number; 0xFFFFFFFF for an inserted AUD, q_t for an inserted set: d_parsed / d_compact
 *                     are carried over with a gather instead of a second parse.
 *   d_nal_au_out[j]   the AU's number within the range, from 0 (what hbs_annexb_to_lenpref takes).
 *   d_au_out[a - first_au]   the input record with first_nal, unit_begin, unit_end and nal_count moved to the output,
 *                     first_vcl + the NALs inserted into the AU unless it is ~0u, HBS_AU_PARAM_SETS or-ed in when a set was
 *                     inserted, everything else copied (what hbs_ts_mux takes).
 * d_index_out is what hbs_index_extract of the output returns, with two exceptions: the filter's, for a short last NAL
 * (hbs_filter_annexb above), and one of its own -- when something is inserted at stream offset 0 and the stream has bytes in
 * front of its first start code, a scan of the output attaches those bytes to the inserted NAL.  Every other insertion point
 * is followed by 00 00.
 *
 * d_summary: nal_count = M, nal_found = n_nals, rbsp_bytes = sum of the output rbsp_len, stream_bytes = output bytes,
 * stop_reason = -1 if M > 0 else 0, reserved[0] = AUDs inserted, reserved[1] = parameter-set NALs inserted, reserved[2] = AUs
 * in the clipped range.
 *   error = HBS_E_ARG when the index is inconsistent by the filter's definition (any entry of the batch), or d_au / d_nal_au
 *   do not tile the batch: first_nal_0 == 0, nal_count >= 1, first_nal_{a+1} == first_nal_a + nal_count_a, the last AU ends
 *   at n_nals, unit_begin == d_index[first_nal - 1].end (0 for NAL 0), unit_end == d_index[first_nal + nal_count - 1].end,
 *   first_vcl is ~0u or below nal_count, d_nal_au[k] names the AU that holds k -- for every AU and NAL of the batch, each
 *   record checked before it is used.  Every count of the summary but nal_found is 0 then.
 *   Otherwise error = HBS_E_CAPACITY when out_cap is below the output, or index_cap < M with any of the three per-NAL tables
 *   given; the counts are right.  On either error nothing is written to any output but the summary.
 * d_out == NULL: plan only -- the summary alone is written, no capacity is looked at.  n_nals == 0 or n_aus == 0 is valid:
 * an empty output, nothing is checked.
 * Refused with HBS_E_ARG at once, before anything is written: unknown flags, n_nals or n_aus above 2^32 - 1, out_cap above
 * 2^46 with a d_out, missing or misaligned pointers.
 * Nothing is stored outside [d_out, d_out + output bytes), the first M entries of the per-NAL tables, the range's entries of
 * d_au_out and the summary; no load touches a 16-byte granule that holds no byte of the stream; no host synchronisation;
 * scratch comes from the context's workspace (48 bytes an AU of the batch, 120 bytes an AU of the range, 8 bytes per 64 KiB of
 * out_cap).
 * Alignment: d_stream, d_out, d_index, d_parsed, d_au, d_au_out, d_summary 16 bytes; d_index_out 8 bytes; d_nal_au,
 * d_nal_src, d_nal_au_out 4 bytes.
 *
 * hbs_aud_nal_host (plain C, no GPU): the seven bytes of the AUD the call inserts in front of an AU with that
 * temporal_id_plus1 and slice_types.  0, or HBS_E_ARG (out NULL).
 */
#define HBS_AUINS_AUD               1u  /* an AUD in front of every AU with a picture that does not begin with one */
#define HBS_AUINS_PARAM_SETS        2u  /* the sets in force in front of every AU with HBS_AU_IRAP                 */
#define HBS_AUINS_PARAM_SETS_FIRST  4u  /* ... and in front of the first AU of the range, whatever it is          */
int hbs_au_insert(hbs_ctx* ctx, const uint8_t* d_stream, uint64_t stream_bytes,
                  const hbs_nal_entry* d_index, const hbs_parsed_nal* d_parsed, uint64_t n_nals,
                  const hbs_access_unit* d_au, const uint32_t* d_nal_au, uint64_t n_aus,
                  uint64_t first_au, uint64_t au_count, uint32_t flags,
                  uint8_t* d_out, uint64_t out_cap,
                  hbs_nal_entry* d_index_out, uint32_t* d_nal_src, uint32_t* d_nal_au_out, uint64_t index_cap,
                  hbs_access_unit* d_au_out, hbs_summary* d_summary);
int hbs_aud_nal_host(int temporal_id_plus1, uint32_t slice_types, uint8_t out[7]);

/* Same, for a batch that continues an earlier one: d_initial_sps_slot (an SPS
 * slot = hevc_sps_t followed at hbs_sps_tables_offset() by its derived RPS
 * tables, hbs_sps_slot_bytes() in all) and d_initial_pps (hevc_pps_t) are the
 * parameter sets in force before NAL 0; NULL = none parsed yet. */
int hbs_parse_headers_ctx(hbs_ctx* ctx, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                          hbs_parsed_nal* d_parsed, uint8_t* d_structs, uint64_t structs_cap,
                          const uint8_t* d_initial_sps_slot, const uint8_t* d_initial_pps, hbs_summary* d_summary);

/* Same, and additionally the per-field trace the reference's read_debug_* readers print
 * (hevc_stream.c:2343-3434): for NAL k, d_trace[k * trace_cap ...] receives one record per syntax
 * element read behind the NAL header, in reading order; d_trace_count[k] = how many it produced
 * (records beyond trace_cap are counted, not stored).  `site` identifies the syntax element (the key
 * of the name table the legacy read_debug_hevc_nal_unit prints with), `pos` the bit position of
 * the RBSP cursor before the read, `value` what was read. */
typedef struct hbs_trace_rec { uint32_t site; uint32_t pos; int32_t value; } hbs_trace_rec;
int hbs_parse_headers_trace(hbs_ctx* ctx, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                            hbs_parsed_nal* d_parsed, uint8_t* d_structs, uint64_t structs_cap,
                            const uint8_t* d_initial_sps_slot, const uint8_t* d_initial_pps,
                            hbs_trace_rec* d_trace, uint32_t trace_cap, uint32_t* d_trace_count, hbs_summary* d_summary);
uint64_t hbs_sps_slot_bytes(void);
/* The same, and what the reference would hold BEHIND the last NAL of the batch, for a caller that goes on NAL by NAL or with
 * another batch (the legacy symbols do: they serve the loop of hevc_analyze.c:135-177 from one batch per buffer): the SPS in
 * force with the 32 rows of the derived RPS tables (hevc_stream.c:26-32) -- each row what the last NAL that wrote it left,
 * also rows beyond the SPS's own sets -- into d_state_sps_slot (hbs_sps_slot_bytes()), and the PPS in force into d_state_pps
 * (sizeof(hevc_pps_t)).  Either may be the buffer the initial context came from.  Both NULL: hbs_parse_headers_trace.
 * summary.reserved[1] != 0: a row depends on a chain of more than three slices' own sets; that row was left untouched.
 * Needs d_structs and n_nals >= 1. */
int hbs_parse_headers_state(hbs_ctx* ctx, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                            hbs_parsed_nal* d_parsed, uint8_t* d_structs, uint64_t structs_cap,
                            const uint8_t* d_initial_sps_slot, const uint8_t* d_initial_pps,
                            hbs_trace_rec* d_trace, uint32_t trace_cap, uint32_t* d_trace_count, hbs_summary* d_summary,
                            uint8_t* d_state_sps_slot, uint8_t* d_state_pps);
/* One NAL at a time, exactly as the reference does it (what the legacy symbols use): with this on, a call with
 * n_nals == 1 and a d_initial_sps_slot treats the RPS tables behind that SPS as THE tables (hevc_stream.c:26-32):
 * an SPS writes its rows into them and leaves the others, a slice's own set lands in them, and a slice that names a
 * row nobody of its SPS wrote reads what is there.  The slot is then read AND written by the call.  Batches
 * (n_nals > 1) parse their NALs independently of one another either way. */
int hbs_ctx_set_sequential_parse(hbs_ctx* ctx, int on);
uint64_t hbs_sps_tables_offset(void);
/* How hbs_emit_annexb works: -1 (default) picked per call -- one single-workgroup launch for a handful of small
 * NALs (<= 256 NALs, <= 32 KiB of RBSP: the legacy rbsp_to_nal); otherwise a single pass: by ARENA TILES when the
 * index's NALs lie back to back in the arena in index order (what hbs_index_extract and hbs_write_headers produce;
 * checked on the device together with a few size limits, hbs_emit.hip: k3t_check; a tile that turns out dense in zero
 * pairs -- padding, cabac_zero_words -- is walked by rows by its own workgroup), else by NALs (items of <= 12 KiB);
 * or, on zero-heavy payload (density probe on the device), count / scan / emit; arenas whose mean NAL is below 448
 * bytes: the arena tiles when they apply (up to 1024 NAL starts per 192 KiB), else a lane per NAL.  0 pins the single pass by NALs,
 * 1 the three steps, 2 the arena tiles whenever the index allows them (whatever the arena's size and density).
 * The bytes are the same whichever runs (h264_nal.c:92-132). */
int hbs_ctx_set_emit_path(hbs_ctx* ctx, int path);
/* Diagnostic: 1 when the arena-tile kernel did the whole of the last hbs_emit_annexb on this context (the index was eligible
 * and no tile was handed to another kernel), 0 when another path did (waits for the call to finish). */
int hbs_ctx_last_emit_by_tiles(hbs_ctx* ctx);

/*
 * Synthetic workload S(seed, n_nals, mode) of SURVEY.md 8(d), generated in HBM:
 * RBSP of NAL k is 8192 + mix(k) % 4097 pseudo-random bytes (mode 0 uniform,
 * mode 1 "zero-heavy": ~10 % 00 and ~5 % 01..03), first bytes 02 01, last byte
 * 80.  Fills d_rbsp (packed) and d_index[k].rbsp_off/rbsp_len; follow with
 * hbs_emit_annexb(..., gap_mode 1, ...) to obtain the Annex-B stream.
 * d_summary->stream_bytes receives the RBSP bytes written.
 */
int hbs_synth_rbsp(hbs_ctx* ctx, uint64_t seed, uint64_t n_nals, int mode,
                   uint8_t* d_rbsp, uint64_t rbsp_cap, hbs_nal_entry* d_index, hbs_summary* d_summary);
uint64_t hbs_synth_rbsp_bound(uint64_t n_nals);

/*
 * K5: the syntax writers behind write_hevc_nal_unit (hevc_stream.c:1249-1327): NAL k's struct
 * (at d_structs + d_parsed[k].struct_off, of the type d_parsed[k] names; layout as hbs_parse_headers
 * leaves it, an SPS followed by its derived tables) is serialised into d_rbsp_out + k * rbsp_cap
 * (rbsp_cap bytes per NAL, zero-filled first; the reference uses size * 3 / 4 of the caller's buffer).
 * Slices are written against the last SPS / PPS in front of them in the batch (or the initial ones).
 * d_written[k]: rc 0 / -1 (unsupported type, or wrote past rbsp_cap), the whole bytes written, and
 * what the reference's writer leaves in h->slice_data->rbsp_size.  hbs_emit_annexb turns the RBSP
 * into NAL bytes (rbsp_to_nal).  Quirks of the reference's writers are kept: see hbs_parse.h.
 */
typedef struct hbs_written_nal { int32_t rc; uint32_t rbsp_size; int32_t slice_data_size; uint32_t pad; } hbs_written_nal;
int hbs_write_headers(hbs_ctx* ctx, const hbs_parsed_nal* d_parsed, uint64_t n_nals, uint8_t* d_structs,
                      const uint8_t* d_initial_sps_slot, const uint8_t* d_initial_pps,
                      uint8_t* d_rbsp_out, uint32_t rbsp_cap, hbs_written_nal* d_written);

/*
 * ---- Several GPUs: one process per GPU, one context each ------------------------------------------
 * Every rank indexes its own bytes; the one exchange of the path is the gather of the NAL index: the counts (8 bytes per
 * rank) to everybody, then exactly count x 32 bytes per rank, to `root` or (root = -1) to every rank, over RCCL (xGMI inside
 * a node).  Stream bytes and RBSP arenas never travel.  RCCL is looked up at run time (librccl.so.1; the copy the process
 * already carries, if any), so the library has no link-time dependency on it.  Environment HBS_RCCL_LIB=<path> (read once, when
 * the first communicator is made) names the library to take RCCL's entry points from instead -- a site's own RCCL build; this
 * project's tests point it at a shared-memory stand-in to run world > 1 on one GPU.  A path that does not load is an error.
 *
 *   hbs_comm_unique_id   rank 0 makes the 128-byte id; the caller hands it to every rank by its own means (MPI, a file, a socket,
 *                        torch.distributed ...)
 *   hbs_comm_create      every rank, collectively: the communicator (ncclCommInitRank)
 *   hbs_comm_adopt       instead: wrap an ncclComm_t the application already owns (same RCCL copy); not destroyed by hbs_comm_destroy
 *   hbs_gather_index     collective, on the context's stream; returns when the sizes are known (one wait for the 8-byte counts),
 *                        the payload then moves asynchronously on that stream.  d_index: this rank's n_local entries;
 *                        stream_base / rbsp_base: added to start, end / rbsp_off of this rank's entries on the way out (0 for
 *                        independent streams; the part's cut offset for parts of ONE stream); d_all (cap_all entries; receivers
 *                        only): the ranks' entries back to back in rank order; counts_out[world] (host): entries per rank.
 *                        Errors are collective: every rank first learns every rank's count, the capacity of every receiver
 *                        and whether its local preparations succeeded (32 bytes per rank, one all-gather), and all take the
 *                        same decision -- HBS_E_CAPACITY on EVERY rank if the entries do not fit some receiver's d_all,
 *                        HBS_E_HIP on every rank if one of them failed -- before any payload call is posted, so that no rank
 *                        is left inside a collective the others never enter.  world <= 1024.
 *   hbs_gather_parts     the same for parts of ONE stream (below): `stopped` = this part's scan ended at an empty NAL
 *                        (hbs_summary.stop_reason == 1).  The reference's loop over the whole stream ends there
 *                        (hevc_analyze.c:135), so the parts behind the first one that stopped contribute no entries
 *                        (counts_out says 0 for them) and the gathered index is the whole stream's.
 */
#define HBS_COMM_ID_BYTES 128
typedef struct hbs_comm hbs_comm;
int  hbs_comm_unique_id(uint8_t id[HBS_COMM_ID_BYTES]);
int  hbs_comm_create(hbs_ctx* ctx, const uint8_t id[HBS_COMM_ID_BYTES], int rank, int world, hbs_comm** out);
int  hbs_comm_adopt(hbs_ctx* ctx, void* nccl_comm, int rank, int world, hbs_comm** out);
void hbs_comm_destroy(hbs_comm* comm);
int  hbs_comm_rank(const hbs_comm* comm);
int  hbs_comm_world(const hbs_comm* comm);
/* how many workgroup slots hbs_ctx_reserve_workgroups should leave free for this communicator's exchange to run beside the
 * next scan: 8 per peer, between 32 and 64 (of 512) */
int  hbs_comm_reserve_hint(const hbs_comm* comm);
int  hbs_gather_index(hbs_ctx* ctx, hbs_comm* comm, const hbs_nal_entry* d_index, uint64_t n_local,
                      uint64_t stream_base, uint64_t rbsp_base, int root,
                      hbs_nal_entry* d_all, uint64_t cap_all, uint64_t* counts_out);
int  hbs_gather_parts(hbs_ctx* ctx, hbs_comm* comm, const hbs_nal_entry* d_index, uint64_t n_local, int stopped,
                      uint64_t stream_base, uint64_t rbsp_base, int root,
                      hbs_nal_entry* d_all, uint64_t cap_all, uint64_t* counts_out);
int  hbs_ctx_device(hbs_ctx* ctx);
/*
 * ONE stream over several GPUs.  A part begins at the first start code (00 00 01) at or after its nominal boundary:
 * hbs_find_cut_host(bytes, n, from) returns that offset in a HOST buffer (plain C, no GPU involved; ~0: none with 8 bytes behind
 * it -- the part in front then runs to the end).  Both neighbours of a boundary apply the same rule to the same bytes, so they
 * agree without a collective.  A rank uploads its part [cut_r, cut_r+1) FOLLOWED BY the next 8 bytes of the stream (they
 * terminate its last NAL as they do in the whole stream, h264_nal.c:64-72), runs hbs_index_extract on that, and drops the NAL the
 * halo opens with hbs_trim_part(part_bytes = cut_r+1 - cut_r): n_kept entries and rbsp_kept arena bytes are the part's.  The last
 * part has no halo and nothing to trim.  hbs_gather_parts(stopped = (stop_reason == 1), stream_base = cut_r, rbsp_base = RBSP bytes
 * of the parts in front or 0) then yields the whole stream's index, empty NALs in the stream included; RBSP arenas stay where they are.
 * (A part whose scan stopped at an empty NAL has nothing to trim either: its walk never reached the halo.)
 */
uint64_t hbs_find_cut_host(const uint8_t* bytes, uint64_t n, uint64_t from);
int  hbs_trim_part(hbs_ctx* ctx, const hbs_nal_entry* d_index, uint64_t nal_count, uint64_t rbsp_bytes, uint64_t part_bytes,
                   uint64_t* n_kept, uint64_t* rbsp_kept);

/* Device-memory helpers for callers without HIP headers (the legacy C layer):
 * allocate / free on the context's GPU, synchronising copies, async fill. */
int hbs_dev_alloc(hbs_ctx* ctx, uint64_t bytes, void** out);
int hbs_dev_free(hbs_ctx* ctx, void* p);
int hbs_copy_to_device(hbs_ctx* ctx, void* d_dst, const void* h_src, uint64_t bytes);
int hbs_copy_to_host(hbs_ctx* ctx, void* h_dst, const void* d_src, uint64_t bytes);
int hbs_fill_device(hbs_ctx* ctx, void* d_dst, int value, uint64_t bytes);
/* page-locked host memory, a host-to-device copy that does not wait (source must be page-locked and
 * stay untouched until the stream has passed it), device-to-device copy on the context's stream */
int hbs_host_alloc(hbs_ctx* ctx, uint64_t bytes, void** out);
int hbs_host_free(hbs_ctx* ctx, void* p);
int hbs_copy_to_device_async(hbs_ctx* ctx, void* d_dst, const void* h_src, uint64_t bytes);
int hbs_copy_device(hbs_ctx* ctx, void* d_dst, const void* d_src, uint64_t bytes);

/*
 * Output buffers placed against the input they are written from.
 *
 * On MI355X a kernel that reads one large buffer and writes another in long bursts (hbs_index_extract: stream -> RBSP arena;
 * hbs_emit_annexb: arena -> stream) runs ~4-5 % slower when both buffers lie in the same one of two classes of physical
 * memory (16 GiB: 6.20 against 5.90 ms; DESIGN.md section 3, profiles/r04/placement_*.txt) -- decided when the buffers are
 * allocated, the same for every offset inside them, and invisible to HIP.  hbs_pair_alloc returns `bytes` of device memory
 * whose placement against `d_peer` (16-byte aligned, its final size and location; contents do not matter and are not changed)
 * has been MEASURED.  Buffers of 1 GiB and more against peers of 512 MiB and more are put together from 1 GiB physical
 * chunks (hipMemCreate / hipMemMap) of a per-device POOL:
 *   - every chunk the pool creates is classed once, by two content-free copies with the kernels' access pattern (half a GiB
 *     each, ~1 ms, on the context's stream) against the pool's reference chunk and against itself;
 *   - each GiB piece of the peer is classed the same way (one copy; by table lookup when the peer is itself such a buffer),
 *     and chunk k of the buffer is one of the class its peer piece is NOT in;
 *   - hbs_pair_free unmaps the buffer and puts its chunks back on the pool's free list, class attached; chunks of the class
 *     nobody wanted stay there too.  A later hbs_pair_alloc takes them: no probes but the peer's, typically 16-20 ms for
 *     16 GiB where the first call of a process takes 0.05-5 s (it has to find memory of both classes: up to `chunks + 88` new
 *     chunks and 128 GiB of unmapped ballast to skip runs of one class, released when the call ends, 24 GiB of the device
 *     left free throughout).
 *   - the free list is bounded: what exceeds HBS_PAIR_POOL_KEEP_GIB (default 48) GiB when a call ends goes back to the driver,
 *     hbs_pair_pool_trim(ctx, keep_bytes) releases on demand, hbs_pair_pool_stats reports.
 * What a caller should know about such a buffer: the size is rounded up to whole GiB; it is virtual-memory-API memory -- no
 * hipFree (hbs_pair_free only), no HIP IPC handle; its addresses come from one 32 TiB reservation per process that is used
 * front to back and never again (a range that had been unmapped and mapped again served stale physical memory on this stack):
 * ~17 GiB of addresses per 16 GiB buffer, about 1 900 such allocations per process, after which hbs_pair_alloc silently takes
 * the plain way below.  One hbs_pair_alloc at a time per process (they share the pool, the address reservation and the probes).
 * Smaller buffers, smaller peers, d_peer == NULL, HBS_PAIR_PLAIN=1, or when the virtual-memory calls fail: ordinary hipMalloc
 * memory -- with a peer to measure against, up to six whole allocations are tried and the one with the most fast pieces kept.
 * hbs_pair_free may be called from any thread (a destructor, a garbage collector): it leaves the caller's current device as it
 * found it and waits only for the context's stream (the whole device when ctx is NULL).
 * Plain hipMalloc / torch buffers keep working everywhere; they land in the slow mode about every other time.  No reference
 * counterpart (the reference's buffers are malloc'ed host memory, hevc_analyze.c:100-103).
 */
typedef struct hbs_pair_report {
    uint32_t chunks;                 /* GiB pieces of the buffer (the last one may be partial)                         */
    uint32_t probed;                 /* probe measurements of this call: peer pieces and NEW chunks                    */
    uint32_t rejected;               /* new chunks of a class nobody wanted (they stay on the pool's free list)        */
    uint32_t accepted_fast;          /* pieces of the returned buffer known to pair fast with their peer piece         */
    uint32_t unprobed_after_budget;  /* pieces of the returned buffer that do not (or were not measured)               */
    uint32_t from_pool;              /* pieces that came off the pool's free list (classed by an earlier call)         */
    uint32_t from_table;             /* peer pieces classed by lookup (the peer is itself a buffer of the pool)        */
    uint32_t reserved;
} hbs_pair_report;
int hbs_pair_alloc(hbs_ctx* ctx, const void* d_peer, uint64_t peer_bytes, uint64_t bytes, void** out, hbs_pair_report* report /* may be NULL */);
int hbs_pair_free(hbs_ctx* ctx, void* ptr);
uint64_t hbs_pair_pool_trim(hbs_ctx* ctx, uint64_t keep_bytes);
int hbs_pair_pool_stats(hbs_ctx* ctx, uint64_t out[4] /* chunks created, chunks classed, free chunks of class 0, of class 1 */);

/* Synchronising copy of a device hbs_summary to the host. */
int hbs_read_summary(hbs_ctx* ctx, const hbs_summary* d_summary, hbs_summary* h_summary);

/* Upper bound of the scratch the context will hold for a stream this long
 * (look-back descriptors; allocated lazily, reused between calls). */
uint64_t hbs_workspace_bytes(uint64_t stream_bytes);

/* Device memory the context itself holds right now (look-back descriptors, run header, padded last tile, the K3 / K4 /
 * index-only workspace, the header windows of hbs_index_parse): grow-only scratch, sized by what the calls so far needed --
 * by the NALs FOUND, never by an index capacity.  Caller-owned buffers (stream, index, arena, structs) are not counted. */
uint64_t hbs_ctx_device_bytes(hbs_ctx* ctx);

/* Legacy single-NAL symbols (h264_stream.h / hevc_stream.h) only.  The derived short-term RPS tables are process state in
 * the reference (file-static, zero at program start, hevc_stream.c:26-32) and device state here; this puts them back to
 * "program start", which the reference can only do by starting a new process.  Not part of the reference's API. */
void hbs_legacy_reset_tables(void);
/* Legacy symbols only, a measuring / testing aid: how the loop of a caller was answered so far -- out[0] batches built (one
 * upload + index + extraction + parse of up to 64 MiB each), [1] reads answered from a batch, [2] reads answered one call at a
 * time, [3] batch builds suppressed by the back-off (a batch that is dropped before the calls answered from it were worth its
 * cost makes the next 1, 2, 4, ... find_nal_unit calls of large buffers go without one; hbs_legacy.c). */
void hbs_legacy_batch_stats(uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
