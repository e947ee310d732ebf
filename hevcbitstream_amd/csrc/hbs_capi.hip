/*
 * hbs_capi.hip -- the extern "C" boundary (include/hevcbitstream_amd.h).
 * Thin: owns the per-GPU context (HIP stream, grow-only scratch) and turns
 * each call into kernel launches.  No CPU implementation of any entry point
 * exists here: without a gfx950 device the context cannot be created.
 */
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include "hbs_scan.h"
#include "hbs_emit_launch.h"
#include "hbs_emit.h"
#include "hbs_parse_launch.h"
#include "hbs_hdrwin.h"
#include "hbs_parse.h"
#include "hbs_parse_compact.h"
#include "hbs_filter.h"
#include "hbs_lenpref.h"
#include "hbs_au.h"
#include "hbs_autimes.h"
#include "hbs_cenc.h"
#include "hbs_cbcs.h"
#include "hbs_ts.h"
#include "hbs_tsmux.h"
#include "hbs_auins.h"
#include "hbs_rtp.h"
#include "hbs_rtpun.h"
#include "hbs_rtpord.h"
#include "hbs_mp4.h"
#include "hbs_mp4rd.h"
#include "hbs_mp4prot.h"
#include "hbs_mp4senc.h"
#include "hbs_mp4stbl.h"
#include "hbs_mp4stblw.h"

constexpr int kTimingRing = 64;       /* timed calls whose event pairs are kept (hbs_ctx_kernel_ms_back) */

struct Buf { void* ptr; uint64_t bytes; };     /* grow-only device memory (grow) */
/* The scratch hbs_ctx_device_bytes counts, each allocated by the first call that needs it:
 * kDesc   look-back words, two per 64 KiB tile of the stream
 * kWs     K3 / generator / parse workspace; the index-only kernels' tile aggregates and elements
 * kAhead  K12's dense tiles counted ahead (streams from 3 GiB up), laid out for ahead_tiles tiles
 * kWs2    hbs_index_parse: header windows and the index that points into them (alive across the parse, which carves kWs)
 * kZeros  sizeof(hevc_sps_t) zero bytes: the "no parameter set yet" structs
 * kFws    hbs_filter_annexb's scratch
 * kAws    hbs_access_units' scratch.  hbs_au_keep uses its first 16 bytes (where hbs_access_units keeps its digest): the calls
 *         of a context are ordered by its one stream, so neither sees the other's data
 * kLws    the scratch of hbs_annexb_to_lenpref and hbs_lenpref_to_annexb
 * kTws    hbs_ts_demux's scratch
 * kMws    hbs_ts_mux's scratch
 * kIws    hbs_au_insert's scratch
 * kRws    hbs_rtp_pack's scratch
 * kUws    hbs_rtp_unpack's scratch
 * kOws    hbs_rtp_order's scratch
 * kPws    hbs_mp4_fragment's scratch
 * kQws    hbs_mp4_samples' scratch
 * kSws    hbs_mp4_stbl_samples' scratch
 * kVws    hbs_mp4_stbl_write's scratch
 * kXws    hbs_au_times' scratch
 * kCws    hbs_cenc_subsamples' scratch
 * kYws    hbs_cenc_crypt's scratch (tables about the samples and the entries; the key is never in it); hbs_cbcs_crypt's too: the
 *         same tables, and the calls of a context are ordered by its one stream
 * kEws    hbs_mp4_protect's scratch
 * kNws    hbs_mp4_senc_samples' scratch */
enum { kDesc, kWs, kAhead, kWs2, kZeros, kFws, kAws, kLws, kTws, kMws, kIws, kRws, kUws, kOws, kPws, kQws, kSws, kVws, kXws, kCws, kYws, kEws, kNws, kBufs };
/* a persistent scan kernel's workgroups: launched, what the GPU holds (`blocks` may be cut: cut_grids), per compute unit */
struct Grid { int blocks, full, per_cu; };

struct hbs_ctx {
    int device;
    int cus;                            /* compute units of `device` */
    hipStream_t own_stream;
    hipStream_t stream;
    Grid grid, grid4, grid6;            /* LDS-image kernel, event-sparse kernel, its 24-row geometry (variant 6) */
    int grid_env, spare_wgs;            /* HBS_GRID_BLOCKS (0: unset); workgroup slots left free for other streams' kernels */
    int exclusive;                      /* hbs_ctx_set_device_exclusive: no other persistent kernel shares the device */
    int variant;                  /* 0 = automatic */
    int last_variant;             /* the kernel the last hbs_index_extract ran (automatic mode: as last read back) */
    int probe_pending;            /* the last hbs_index_extract chose on the device: hbs_ctx_last_kernel reads the probe back, at every call of it */
    int last_index_only;          /* the last hbs_index_extract had no arena: its sparse kernel is the streaming one (5) */
    int parse_sequential;         /* hbs_ctx_set_sequential_parse */
    int count_ahead;              /* hbs_ctx_set_count_ahead: 0 never, 1 streams from 3 GiB up, 2 always */
    uint64_t ingest_window_max;   /* hbs_ctx_set_ingest_window_max (0: the default) */
    void* attachment;             /* state another translation unit keeps with the context (the windowed ingest's buffers) */
    void (*attachment_free)(void*);
    int emit_blocks, emit_two_pass;   /* K3: resident workgroups of the single-pass kernel; 1 = use the older three-step path */
    int emit_tile_blocks, emit_tiles; /* ... of the arena-tile kernel; 0 never / 1 when eligible / 2 pinned */
    int emit_path_set;                /* hbs_ctx_set_emit_path was called: the environment no longer decides */
    const uint32_t* last_emit_tflag;  /* the last hbs_emit_annexb's verdict words: a COPY in emit_verdict (the words themselves live in the shared
                                         workspace, which the next call of any kind overwrites or reallocates); null: no verdict (small path) */
    Buf emit_verdict;                 /* 16 bytes of device memory owned by the context (hbs_ctx_device_bytes never counted them) */
    uint32_t emit_calls;              /* hbs_emit_annexb calls so far: stamps the dense tiles counted ahead (never 0) */
    hbs::RunHeader* hdr;
    uint8_t* tail;                      /* padded copy of the stream's last tile (event-sparse kernel) */
    Buf buf[kBufs];
    uint64_t ahead_tiles;               /* 192 KiB tiles buf[kAhead] is laid out for */
    /* optional timing of the dominant kernel */
    int timing; int ev_valid;                             /* ev_valid: a timed call has taken a slot since timing was switched on */
    hipEvent_t ring0[kTimingRing], ring1[kTimingRing];    /* event pairs of the last kTimingRing timed calls */
    unsigned long long timed_calls;                       /* the last one used slot (timed_calls - 1) % kTimingRing */
    char err[256];
};

namespace {

int fail(hbs_ctx* c, hipError_t e, const char* what)
{
    if (c) snprintf(c->err, sizeof(c->err), "%s: %s", what, hipGetErrorString(e));
    return HBS_E_HIP;
}

bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

/* a call's pointers, grouped by the alignment they must have (null is aligned): true, with `msg` as the error's text, when one
 * of them is not */
using Ptrs = std::initializer_list<const void*>;
bool misaligned_refused(hbs_ctx* c, const char* msg, Ptrs by16, Ptrs by8, Ptrs by4 = {})
{
    bool bad = false;
    for (const void* p : by16) bad = bad || misaligned(p, 15);
    for (const void* p : by8) bad = bad || misaligned(p, 7);
    for (const void* p : by4) bad = bad || misaligned(p, 3);
    if (bad) snprintf(c->err, sizeof(c->err), "%s", msg);
    return bad;
}

/* a call whose out_cap sizes its scratch and grid: true, with the error's text, when it asks for more than kOutCapMax */
bool out_cap_refused(hbs_ctx* c, const void* d_out, uint64_t out_cap)
{
    if (!d_out || out_cap <= hbs::kOutCapMax) return false;
    snprintf(c->err, sizeof(c->err), "out_cap sizes the call's scratch and grid: at most 2^46");
    return true;
}

/* makes `b` hold `bytes` at least.  1: it grew (what it held is gone), 0: it was large enough, < 0: the call's return code */
int grow(hbs_ctx* c, Buf& b, uint64_t bytes, const char* what)
{
    if (bytes <= b.bytes) return 0;
    if (b.ptr) { (void)hipStreamSynchronize(c->stream); (void)hipFree(b.ptr); b.ptr = nullptr; b.bytes = 0; }
    const hipError_t e = hipMalloc(&b.ptr, bytes);
    if (e != hipSuccess) return fail(c, e, what);
    b.bytes = bytes;
    return 1;
}

/* a call's workspace in `b`: `lay` fills the call's *Args through the cursor, once to learn the size and again on `b` grown to
 * it.  Returns as grow does. */
template <class Lay> int carve(hbs_ctx* c, Buf& b, const char* what, Lay lay)
{
    hbs::Carver w{nullptr, 0};
    lay(w);
    const int rc = grow(c, b, w.at, what);
    if (rc < 0) return rc;
    w = hbs::Carver{static_cast<uint8_t*>(b.ptr), 0};
    lay(w);
    return rc;
}

int ensure_zeros(hbs_ctx* c)
{
    const uint64_t zb = (sizeof(hevc_sps_t) + 255) & ~(uint64_t)255;
    const int rc = grow(c, c->buf[kZeros], zb, "hipMalloc(zero structs)");
    if (rc <= 0) return rc;
    const hipError_t e = hipMemsetAsync(c->buf[kZeros].ptr, 0, zb, c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "hipMemsetAsync(zero structs)");
}

/* the call takes its slot of the timing ring: the event pair around its kernels */
void take_timing_slot(hbs_ctx* c, hipEvent_t* begin, hipEvent_t* end)
{
    const int slot = (int)(c->timed_calls % kTimingRing);
    *begin = c->ring0[slot]; *end = c->ring1[slot];
    c->timed_calls += 1;
    c->ev_valid = 1;
}

/* The tail of a plan-and-copy call, behind its argument checks and hipSetDevice: the scratch carved into `a` by the call's lay_*
 * (a failed allocation returns at once and takes no slot), then a slot of the timing ring around all of the call's kernels, then
 * the launch.  `name`: the launcher's, for hbs_last_error. */
template <class Args>
int carve_and_launch(hbs_ctx* c, Buf& scratch, const char* what, Args& a, void (*lay)(hbs::Carver&, Args&),
                     hipError_t (*launch)(const Args&, hipStream_t), const char* name)
{
    const int rc = carve(c, scratch, what, [&](hbs::Carver& w) { lay(w, a); });
    if (rc < 0) return rc;
    if (c->timing) take_timing_slot(c, &a.ev_begin, &a.ev_end);
    const hipError_t e = launch(a, c->stream);
    return e == hipSuccess ? 0 : fail(c, e, name);
}

/* what each scan kernel launches: what the GPU holds less the slots left free, under the HBS_GRID_BLOCKS debugging cap (a ceiling
 * of its own: reserving workgroups never raises it) */
void cut_grids(hbs_ctx* c)
{
    for (Grid* g : {&c->grid, &c->grid4, &c->grid6}) {
        g->blocks = g->full - c->spare_wgs > 1 ? g->full - c->spare_wgs : 1;
        if (c->grid_env > 0 && c->grid_env < g->blocks) g->blocks = c->grid_env;
    }
}

int parse_impl(hbs_ctx* c, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
               hbs_parsed_nal* d_parsed, uint8_t* d_structs, uint64_t structs_cap,
               const uint8_t* d_initial_sps_slot, const uint8_t* d_initial_pps,
               hbs_trace_rec* d_trace, uint32_t trace_cap, uint32_t* d_trace_count, hbs_summary* d_summary,
               uint8_t* d_state_sps_slot, uint8_t* d_state_pps,
               hbs_slice_compact* d_compact, const uint64_t* d_want, uint64_t n_want)
{
    static_assert(sizeof(hbs_slice_compact) == sizeof(hbs::SliceCompact), "public record == kernel record");
    if ((d_state_sps_slot == nullptr) != (d_state_pps == nullptr)) return HBS_E_ARG;
    if (d_state_sps_slot && (!d_structs || !n_nals)) return HBS_E_ARG;
    static_assert(sizeof(hbs_trace_rec) == sizeof(hbs::TraceRec), "public record == kernel record");
    static_assert(sizeof(hbs_parsed_nal) == sizeof(hbs::ParsedNal), "public record == kernel record");
    if (!c || !d_summary || (n_nals && (!d_rbsp || !d_index || !d_parsed))) return HBS_E_ARG;
    if (misaligned(d_structs, 15)) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    int rc = ensure_zeros(c);
    if (rc) return rc;
    hbs::ParseArgs a;
    a.rbsp = d_rbsp; a.index = d_index; a.n = n_nals;
    a.parsed = reinterpret_cast<hbs::ParsedNal*>(d_parsed);
    a.structs = d_structs; a.structs_cap = d_structs ? structs_cap : 0; a.summary = d_summary;
    a.zeros = static_cast<const uint8_t*>(c->buf[kZeros].ptr);
    a.initial_sps_slot = d_initial_sps_slot;
    a.initial_pps = d_initial_pps;
    a.trace = reinterpret_cast<hbs::TraceRec*>(d_trace); a.trace_cap = trace_cap; a.trace_count = d_trace_count;
    a.state_sps_slot_out = d_state_sps_slot; a.state_pps_out = d_state_pps;
    a.compact = reinterpret_cast<hbs::SliceCompact*>(d_compact); a.want_list = d_want; a.want_n = d_compact ? n_want : 0;
    a.sequential = (d_state_sps_slot || d_compact) ? 0 : c->parse_sequential;
    rc = carve(c, c->buf[kWs], "hipMalloc(workspace)", [&](hbs::Carver& w) { hbs::lay_parse(w, a); });
    if (rc < 0) return rc;
    hipError_t e = hbs::launch_parse_headers(a, c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "launch_parse_headers");
}

int index_parse_impl(hbs_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes,
                     hbs_nal_entry* d_index, uint64_t index_cap, uint32_t header_window,
                     hbs_parsed_nal* d_parsed, hbs_slice_compact* d_compact, uint8_t* d_structs, uint64_t structs_cap, uint64_t* d_payload_off,
                     hbs_summary* d_scan_summary, hbs_summary* d_parse_summary, uint64_t* nal_count_out)
{
    if (!c || !d_scan_summary || !d_parse_summary || !d_index || !index_cap || !d_parsed) return HBS_E_ARG;
    if (header_window == 0) header_window = 512;
    if (header_window < 64 || header_window > (1u << 16) || (header_window & 15u)) return HBS_E_ARG;
    /* what the parse behind the scan would refuse is refused here, before the scan has written the index and its summary */
    if (misaligned(d_structs, 15)) return HBS_E_ARG;
    /* 1. find_nal_unit over the stream: no arena */
    int rc = hbs_index_extract(c, d_stream, stream_bytes, d_index, index_cap, nullptr, 0, d_scan_summary);
    if (rc) return rc;
    /* the parse's launches are sized by the number of NALs: the one wait of the call */
    hbs_summary s;
    rc = hbs_read_summary(c, d_scan_summary, &s);
    if (rc) return rc;
    if (nal_count_out) *nal_count_out = s.nal_count;
    if (s.error) return s.error;
    const uint64_t nals = s.nal_count;
    /* 2. the bytes the parse can look at, stripped into windows */
    hbs::HdrWinArgs a;
    /* everything below is sized by the NALs FOUND (known since the wait above), not by the caller's index capacity: a default
     * capacity of stream_bytes / 64 entries would ask for 137 GB of windows on a 16 GiB stream (round 3's advice) */
    const uint64_t slots = nals ? nals : 1;
    a.stream = d_stream; a.index = d_index; a.nals = nals; a.index_cap = slots; a.window = header_window;
    a.arena_bytes = hbs::hdrwin_arena_bytes(slots, header_window, stream_bytes);
    rc = carve(c, c->buf[kWs2], "hipMalloc(header windows)", [&](hbs::Carver& w) { hbs::lay_hdrwin(w, a); });
    if (rc < 0) return rc;
    hipError_t e = hbs::launch_hdr_strip(a, c->stream);
    if (e != hipSuccess) return fail(c, e, "launch_hdr_strip");
    /* 3. K4 on the windows, 4. slice_data_size against the real lengths, windows that were too small reported */
    rc = d_compact ? hbs_parse_headers_compact(c, a.arena, a.idx2, nals, d_parsed, d_compact, d_structs, structs_cap, nullptr, nullptr, d_parse_summary)
                   : hbs_parse_headers(c, a.arena, a.idx2, nals, d_parsed, d_structs, structs_cap, d_parse_summary);
    if (rc) return rc;
    e = hbs::launch_hdr_fix(a, d_parsed, d_parse_summary, reinterpret_cast<unsigned long long*>(d_payload_off), c->stream, d_compact ? 1 : 0);
    return e == hipSuccess ? 0 : fail(c, e, "launch_hdr_fix");
}

} // namespace

extern "C" {

const char* hbs_version(void)
{
    return "hevcbitstream_amd 0.6 (gfx950 HIP; K12 fused scan/index/extract)";
}

int hbs_ctx_create(hbs_ctx** out, int device)
{
    if (!out) return HBS_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return HBS_E_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return HBS_E_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return HBS_E_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fprintf(stderr, "hevcbitstream_amd: device %d is %s; this library carries gfx950 code only\n", device, prop.gcnArchName);
        return HBS_E_NO_DEVICE;
    }
    hbs_ctx* c = new (std::nothrow) hbs_ctx();
    if (!c) return HBS_E_HIP;
    memset(c, 0, sizeof(*c));
    c->device = device;
    c->cus = prop.multiProcessorCount;
    const bool ok = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) == hipSuccess &&
                    hipMalloc(reinterpret_cast<void**>(&c->hdr), sizeof(hbs::RunHeader)) == hipSuccess &&
                    hipMalloc(reinterpret_cast<void**>(&c->tail), (size_t)hbs::scan4_tail_bytes()) == hipSuccess &&
                    (c->grid.full = hbs::scan_grid_blocks(device, &c->grid.per_cu)) > 0 &&
                    (c->grid4.full = hbs::scan4_grid_blocks(device, &c->grid4.per_cu)) > 0 &&
                    (c->grid6.full = hbs::scan4r24_grid_blocks(device, &c->grid6.per_cu)) > 0;
    c->stream = c->own_stream;
    if (!ok) { hbs_ctx_destroy(c); return HBS_E_HIP; }
    const char* g = getenv("HBS_GRID_BLOCKS");          /* debugging aid: 1 = fully sequential tiles */
    const int cap = g ? atoi(g) : 0;
    c->grid_env = cap > 0 ? cap : 0;
    cut_grids(c);
    const char* ca = getenv("HBS_COUNT_AHEAD");
    c->count_ahead = (ca && ca[0] >= '0' && ca[0] <= '2') ? ca[0] - '0' : 1;
    const char* kv = getenv("HBS_KERNEL");              /* 0 automatic, 2 LDS-image, 4 event-sparse, 5 index-only streaming, 6 event-sparse with 24 rows */
    const int k = kv ? atoi(kv) : 0;
    c->variant = (k == 2 || k == 4 || k == 5 || k == 6) ? k : 0;
    c->last_variant = c->variant ? c->variant : 4;
    *out = c;
    return 0;
}

/* also the one failure path of hbs_ctx_create: whatever the context does not hold yet is null */
void hbs_ctx_destroy(hbs_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->attachment && c->attachment_free) c->attachment_free(c->attachment);
    if (c->hdr) (void)hipFree(c->hdr);
    if (c->tail) (void)hipFree(c->tail);
    if (c->emit_verdict.ptr) (void)hipFree(c->emit_verdict.ptr);
    for (Buf& b : c->buf) if (b.ptr) (void)hipFree(b.ptr);
    if (c->ring0[0]) for (int i = 0; i < kTimingRing; ++i) { (void)hipEventDestroy(c->ring0[i]); (void)hipEventDestroy(c->ring1[i]); }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

/* internal (hbs_place.hip): what hbs_last_error will say; not exported */
__attribute__((visibility("hidden"))) void hbs_ctx_set_error(hbs_ctx* c, const char* what, int hip_error)
{
    if (c) snprintf(c->err, sizeof(c->err), "%s: %s", what, hipGetErrorString((hipError_t)hip_error));
}
__attribute__((visibility("hidden"))) uint64_t hbs_ctx_ingest_window_max(hbs_ctx* c) { return c ? c->ingest_window_max : 0; }
/* internal (hbs_ingest.hip): one object kept alive with the context, freed with it; not exported */
__attribute__((visibility("hidden"))) void* hbs_ctx_attachment(hbs_ctx* c) { return c ? c->attachment : nullptr; }
__attribute__((visibility("hidden"))) void hbs_ctx_attach(hbs_ctx* c, void* p, void (*free_fn)(void*))
{
    if (!c) return;
    if (c->attachment && c->attachment_free && c->attachment != p) c->attachment_free(c->attachment);
    c->attachment = p; c->attachment_free = free_fn;
}

int hbs_ctx_set_stream(hbs_ctx* c, void* s)
{
    if (!c) return HBS_E_ARG;
    c->stream = reinterpret_cast<hipStream_t>(s);     /* NULL = the HIP null stream */
    return 0;
}

int hbs_ctx_enable_timing(hbs_ctx* c, int on)
{
    if (!c) return HBS_E_ARG;
    if (on && !c->ring0[0]) {
        if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
        for (int i = 0; i < kTimingRing; ++i)
            if (hipEventCreate(&c->ring0[i]) != hipSuccess || hipEventCreate(&c->ring1[i]) != hipSuccess) {
                /* all or nothing: ring0[0] != null means "the whole ring exists" everywhere else */
                for (int j = 0; j <= i; ++j) {
                    if (c->ring0[j]) (void)hipEventDestroy(c->ring0[j]);
                    if (c->ring1[j]) (void)hipEventDestroy(c->ring1[j]);
                    c->ring0[j] = nullptr; c->ring1[j] = nullptr;
                }
                c->timing = 0; c->ev_valid = 0;
                return HBS_E_HIP;
            }
    }
    c->timing = on ? 1 : 0;
    c->ev_valid = 0;
    c->timed_calls = 0;
    return 0;
}

/* the timed call `back` calls ago (0 = the last one); the ring keeps kTimingRing of them */
int hbs_ctx_kernel_ms_back(hbs_ctx* c, int back, float* ms)
{
    if (!c || !ms || !c->ev_valid || back < 0 || back >= kTimingRing || (unsigned long long)back >= c->timed_calls) return HBS_E_ARG;
    const int slot = (int)((c->timed_calls - 1 - (unsigned long long)back) % kTimingRing);
    hipError_t e = hipEventSynchronize(c->ring1[slot]);
    if (e != hipSuccess) return fail(c, e, "hipEventSynchronize");
    e = hipEventElapsedTime(ms, c->ring0[slot], c->ring1[slot]);
    return e == hipSuccess ? 0 : fail(c, e, "hipEventElapsedTime");
}

int hbs_ctx_kernel_ms(hbs_ctx* c, float* ms) { return hbs_ctx_kernel_ms_back(c, 0, ms); }

/* The scan kernels are persistent: their workgroups fill the GPU (the event-sparse kernel's 512 use every register), so a kernel
 * of another stream -- RCCL's, in the index gather of the multi-GPU path -- finds no CU until the scan ends, and a "pipelined"
 * exchange runs in the gaps between scans.  Leaving a few workgroup slots free lets it run beside the scan. */
int hbs_ctx_reserve_workgroups(hbs_ctx* c, int spare)
{
    if (!c || spare < 0) return HBS_E_ARG;
    c->spare_wgs = spare;
    cut_grids(c);
    return 0;
}

/* Default 0: every tile of the persistent kernels (scan + extraction, arena-tile emit) comes by ticket, which needs no assumption
 * about what else runs on the device.  1: the caller says this context's calls are the only persistent kernels on the device while
 * they run; a workgroup's first tile is then its number (no queue of 512 atomics on one address at the start of a call: ~1 % of a
 * 1 GiB call).  Two contexts or processes that scan ONE device at the same time must leave it at 0: with static first tiles each
 * could hold workgroup slots the other's low-numbered workgroups need, and wait until the look-back guard gives up (HBS_E_TIMEOUT). */
int hbs_ctx_set_device_exclusive(hbs_ctx* c, int on)
{
    if (!c || (on != 0 && on != 1)) return HBS_E_ARG;
    c->exclusive = on;
    return 0;
}


int hbs_ctx_grid(hbs_ctx* c, int* blocks, int* blocks_per_cu)
{
    if (!c) return HBS_E_ARG;
    const int v = c->variant ? c->variant : c->last_variant;
    const Grid& g = (v == 4) ? c->grid4 : (v == 6) ? c->grid6 : c->grid;
    if (blocks) *blocks = g.blocks;
    if (blocks_per_cu) *blocks_per_cu = g.per_cu;
    return 0;
}

int hbs_ctx_set_kernel(hbs_ctx* c, int variant)
{
    if (!c || variant < 0 || variant == 1 || variant == 3 || variant > 6) return HBS_E_ARG;
    c->variant = variant;
    if (variant) c->last_variant = variant;
    return 0;
}

int hbs_ctx_get_kernel(hbs_ctx* c) { return c ? c->variant : HBS_E_ARG; }

int hbs_ctx_set_count_ahead(hbs_ctx* c, int mode)
{
    if (!c || mode < 0 || mode > 2) return HBS_E_ARG;
    c->count_ahead = mode;
    return 0;
}
int hbs_ctx_device(hbs_ctx* c) { return c ? c->device : HBS_E_ARG; }

int hbs_ctx_set_sequential_parse(hbs_ctx* c, int on)
{
    if (!c) return HBS_E_ARG;
    c->parse_sequential = on ? 1 : 0;
    return 0;
}

int hbs_ctx_set_ingest_window_max(hbs_ctx* c, uint64_t max_window_bytes)
{
    if (!c) return HBS_E_ARG;
    c->ingest_window_max = max_window_bytes;
    return 0;
}

int hbs_ctx_set_emit_path(hbs_ctx* c, int path)
{
    if (!c || path < -1 || path > 2) return HBS_E_ARG;
    /* -1: everything picked per call; 0: the item kernel (k3_fused); 1: count / scan / emit; 2: the arena-tile kernel whenever the
     * index allows it (the item kernel when it does not) */
    c->emit_two_pass = path == 2 ? 0 : path;
    c->emit_tiles = path == 2 ? 2 : (path == -1 ? 1 : 0);
    c->emit_path_set = 1;
    return 0;
}

/* 1: the arena-tile kernel did the whole of the last hbs_emit_annexb (eligible index, no tile handed over); 0: another path; waits */
int hbs_ctx_last_emit_by_tiles(hbs_ctx* c)
{
    if (!c) return HBS_E_ARG;
    if (!c->last_emit_tflag) return 0;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    uint32_t f[4] = {0, 0, 0, 0};
    hipError_t e = hipMemcpyAsync(f, c->last_emit_tflag, sizeof(f), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, e, "read-back of the emit verdict");
    return (f[1] == 1u && f[0] == 0u && f[3] == 0u && f[2] == 0u) ? 1 : 0;
}

int hbs_ctx_last_kernel(hbs_ctx* c)
{
    if (!c) return HBS_E_ARG;
    if (c->variant) return (c->variant == 5 && !c->last_index_only) ? 4 : c->variant;
    if (!c->probe_pending) return c->last_variant;
    /* automatic mode: the choice was made on the device; read the probe's counts back.  Every time: a call captured in a HIP graph
     * runs again at each replay without the host side of hbs_index_extract, so a value kept from the first read-back would be the
     * kernel of an earlier replay */
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::RunHeader h;
    hipError_t e = hipMemcpyAsync(&h, c->hdr, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, e, "read-back of the density probe");
    uint64_t chunks = 0, flagged = 0;
    for (int i = 0; i < 64; ++i) { chunks += h.probe_slot[i][0]; flagged += h.probe_slot[i][1]; }
    c->last_variant = hbs::probe_variant((uint32_t)chunks, (uint32_t)flagged, c->last_index_only != 0);
    return c->last_variant;
}

int hbs_ctx_use_own_stream(hbs_ctx* c)
{
    if (!c) return HBS_E_ARG;
    c->stream = c->own_stream;
    return 0;
}

void* hbs_ctx_get_stream(hbs_ctx* c) { return c ? reinterpret_cast<void*>(c->stream) : nullptr; }

int hbs_ctx_synchronize(hbs_ctx* c)
{
    if (!c) return HBS_E_ARG;
    hipError_t e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "hipStreamSynchronize");
}

const char* hbs_last_error(hbs_ctx* c) { return c ? c->err : "no context"; }

uint64_t hbs_ctx_device_bytes(hbs_ctx* c)
{
    if (!c) return 0;
    uint64_t sum = sizeof(hbs::RunHeader) + hbs::scan4_tail_bytes();
    for (const Buf& b : c->buf) sum += b.bytes;
    return sum;
}

uint64_t hbs_workspace_bytes(uint64_t stream_bytes)
{
    return ((stream_bytes + hbs::kTileBytes - 1) / hbs::kTileBytes + 1) * 16 + sizeof(hbs::RunHeader);
}

int hbs_index_extract(hbs_ctx* c, const uint8_t* d_stream, uint64_t n,
                      hbs_nal_entry* d_index, uint64_t index_cap,
                      uint8_t* d_rbsp, uint64_t rbsp_cap, hbs_summary* d_summary)
{
    if (!c || !d_summary || (n && !d_stream) || (index_cap && !d_index)) return HBS_E_ARG;
    if (misaligned(d_stream, 15) || misaligned(d_rbsp, 15) || misaligned(d_index, 7)) {
        snprintf(c->err, sizeof(c->err), "stream/rbsp pointers must be 16-byte aligned");
        return HBS_E_ARG;
    }
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    int rc = grow(c, c->buf[kDesc], ((n + hbs::kTileBytes - 1) / hbs::kTileBytes + 1) * 16, "hipMalloc(look-back descriptors)");
    if (rc < 0) return rc;
    hbs::ScanArgs a;
    a.stream = d_stream; a.n = n;
    a.index = d_index; a.index_cap = index_cap;
    a.rbsp = d_rbsp; a.rbsp_cap = d_rbsp ? rbsp_cap : 0;
    a.desc = static_cast<unsigned long long*>(c->buf[kDesc].ptr); a.hdr = c->hdr; a.tail = c->tail; a.summary = d_summary;
    a.ws5 = nullptr;
    if (!d_rbsp && n) {                                       /* the index-only kernels keep tile aggregates and elements between their passes */
        rc = grow(c, c->buf[kWs], hbs::scan5_workspace_bytes(n), "hipMalloc(workspace)");
        if (rc < 0) return rc;
        a.ws5 = c->buf[kWs].ptr;
    }
    a.ahead_cand = nullptr; a.ahead_tab = nullptr; a.ahead_list = nullptr; a.ahead_ctl = nullptr;
    if (d_rbsp && (c->count_ahead == 2 || (c->count_ahead == 1 && hbs::scan4_counts_ahead(n))) && n > (uint64_t)hbs::scan4_tile_bytes() &&
        (c->variant == 0 || c->variant == 4 || c->variant == 5) /* (6: the 24-row geometry counts nothing ahead) */ && !hbs::scan_takes_small_path(n, index_cap, c->variant)) {
        /* K12's dense tiles counted ahead.  What the tiles' words carry from one call to the next stays where it is: the layout
         * is that of the longest stream so far */
        const uint64_t tiles = (n + (uint64_t)hbs::scan4_tile_bytes() - 1) / (uint64_t)hbs::scan4_tile_bytes();
        const uint64_t room = tiles > c->ahead_tiles ? tiles : c->ahead_tiles;
        uint64_t cleared = 0;
        rc = carve(c, c->buf[kAhead], "hipMalloc(count-ahead table)", [&](hbs::Carver& w) { cleared = hbs::lay_scan_ahead(w, a, room); });
        if (rc < 0) return rc;
        if (rc) {
            const hipError_t e = hipMemsetAsync(c->buf[kAhead].ptr, 0, cleared, c->stream);
            if (e != hipSuccess) return fail(c, e, "hipMemsetAsync(count-ahead words)");
            c->ahead_tiles = room;
        }
    }
    c->last_index_only = (hbs::scan_uses_index_only(n, c->variant, d_rbsp) && !hbs::scan_takes_small_path(n, index_cap, c->variant)) ? 1 : 0;
    a.variant = c->variant;
    a.cus = c->cus;
    a.grid_blocks = c->grid.blocks; a.grid_blocks4 = c->grid4.blocks; a.grid_blocks4r24 = c->grid6.blocks; a.spare_wgs = c->spare_wgs; a.first_static = c->exclusive;
    c->probe_pending = (c->variant == 0 && n) ? 1 : 0;
    if (hbs::scan_takes_small_path(n, index_cap, c->variant)) { c->probe_pending = 0; c->last_variant = 2; }
    a.ev_begin = nullptr; a.ev_end = nullptr;
    if (c->timing && n) take_timing_slot(c, &a.ev_begin, &a.ev_end);
    else c->ev_valid = c->ev_valid && c->timing;             /* a call of no bytes launches nothing: the last timed call stays the one reported */
    hipError_t e = hbs::launch_scan_extract(a, c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "launch_scan_extract");
}

int hbs_emit_annexb(hbs_ctx* c, const uint8_t* d_rbsp, uint64_t rbsp_bytes,
                    const hbs_nal_entry* d_index_in, uint64_t n_nals, int gap_mode,
                    uint8_t* d_out, uint64_t out_cap, hbs_nal_entry* d_index_out, hbs_summary* d_summary)
{
    if (!c || !d_summary || (n_nals && (!d_rbsp || !d_index_in || !d_out))) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::EmitArgs a;
    a.rbsp = d_rbsp; a.rbsp_bytes = rbsp_bytes; a.index_in = d_index_in; a.n = n_nals; a.gap_mode = gap_mode;
    a.out = d_out; a.out_cap = out_cap; a.index_out = d_index_out; a.summary = d_summary;
    /* NALs that do not overlap add up to at most rbsp_bytes; an index whose NALs add up to more gets HBS_E_CAPACITY */
    a.items_cap = hbs::emit_items_bound(n_nals, out_cap < rbsp_bytes ? out_cap : rbsp_bytes);
    a.first_cap = a.cand_cap = rbsp_bytes / (192u * 1024u) + 4;          /* arena tiles of the tile kernel (hbs_emit.hip: kTTileBytes) */
    int rc = carve(c, c->buf[kWs], "hipMalloc(workspace)", [&](hbs::Carver& w) { hbs::lay_emit(w, a); });
    if (rc < 0) return rc;
    if (c->emit_blocks <= 0) {
        c->emit_blocks = hbs::emit_grid_blocks(c->device);
        if (c->emit_blocks <= 0) return fail(c, hipErrorUnknown, "occupancy query of the emit kernel");
        const char* tp = getenv("HBS_EMIT_TWO_PASS");        /* 1 / 0 pin a way; default: picked on the device */
        if (!c->emit_path_set) { c->emit_two_pass = !tp ? -1 : (atoi(tp) == 1 ? 1 : 0); c->emit_tiles = !tp ? 1 : 0; }
        c->emit_tile_blocks = hbs::emit_tile_grid_blocks(c->device);
        if (c->emit_tile_blocks <= 0) return fail(c, hipErrorUnknown, "occupancy query of the arena-tile emit kernel");
    }
    /* dense tiles counted ahead of the tile kernel (k3t_sample + a pass over the tiles it lists): from 3 GiB of arena up, as the scan's
     * (hbs_ctx_set_count_ahead: 0 never, 1 from 3 GiB, 2 always).  Until round 6 every call paid for it -- two launches, 11.5 us of a
     * 1 GiB call's 445 with nothing listed -- where mixed content is as unlikely as in the scan. */
    if (c->count_ahead == 0 || (c->count_ahead == 1 && !hbs::scan4_counts_ahead(rbsp_bytes))) a.dz_table = nullptr;
    c->emit_calls += 1; if (c->emit_calls == 0) c->emit_calls = 1;
    a.call_no = c->emit_calls;
    a.first_static = c->exclusive;
    a.tiles = c->emit_tiles; a.tile_blocks = c->emit_tile_blocks;
    a.grid_blocks = c->emit_blocks; a.two_pass = c->emit_two_pass; a.cus = c->cus;
    rc = grow(c, c->emit_verdict, 16, "hipMalloc(emit verdict)");
    if (rc < 0) return rc;
    /* the verdict words leave the shared workspace with the call's last kernel (round 4's advice: hbs_ctx_last_emit_by_tiles after
     * any other call read bytes that call had overwritten, or a freed workspace); the one-launch small path writes none */
    a.verdict_out = static_cast<uint32_t*>(c->emit_verdict.ptr);
    c->last_emit_tflag = hbs::emit_takes_small_path(a.n, a.rbsp_bytes, a.two_pass) ? nullptr : a.verdict_out;
    hipError_t e = hbs::launch_emit_annexb(a, c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "launch_emit_annexb");
}

int hbs_filter_annexb(hbs_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes,
                      const hbs_nal_entry* d_index, uint64_t n_nals,
                      const hbs_nal_filter* rule, const uint8_t* d_keep,
                      uint8_t* d_out, uint64_t out_cap,
                      hbs_nal_entry* d_index_out, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_nal_filter) == 24, "hbs_nal_filter layout");
    if (!c || !d_summary || (rule == nullptr) == (d_keep == nullptr)) return HBS_E_ARG;
    if (n_nals && (!d_index || (stream_bytes && !d_stream))) return HBS_E_ARG;
    if (misaligned_refused(c, "stream/output pointers must be 16-byte aligned, index pointers 8-byte aligned",
                           {d_stream, d_out}, {d_index, d_index_out})) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    const uint64_t reach = d_out ? (out_cap < stream_bytes ? out_cap : stream_bytes) : 0;    /* the output is at most this long */
    hbs::FilterArgs a;
    memset(&a, 0, sizeof(a));
    a.n = stream_bytes; a.index = d_index; a.n_nals = n_nals;
    if (rule) { a.rule = *rule; a.use_rule = 1; }
    a.keep = d_keep;
    a.out_cap = out_cap; a.index_out = d_index_out; a.summary = d_summary;
    a.t.src = d_stream; a.t.out = d_out; a.t.tiles = hbs::piece_tiles(reach);
    return carve_and_launch(c, c->buf[kFws], "hipMalloc(filter scratch)", a, hbs::lay_filter, hbs::launch_filter_annexb, "launch_filter_annexb");
}

int hbs_annexb_to_lenpref(hbs_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes,
                          const hbs_nal_entry* d_index, uint64_t n_nals, const uint8_t* d_keep, int length_size,
                          const uint32_t* d_nal_au, uint64_t n_aus, uint64_t* d_sample_off,
                          uint8_t* d_out, uint64_t out_cap, hbs_nal_entry* d_index_out, hbs_summary* d_summary)
{
    if (!c || !d_summary || (length_size != 1 && length_size != 2 && length_size != 4)) return HBS_E_ARG;
    if (n_nals && (!d_index || (stream_bytes && !d_stream))) return HBS_E_ARG;
    if (misaligned_refused(c, "stream/output/summary pointers must be 16-byte aligned, index and sample table 8-byte, AU numbers 4-byte",
                           {d_stream, d_out, d_summary}, {d_index, d_index_out, d_sample_off}, {d_nal_au})) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::A2lArgs a;
    memset(&a, 0, sizeof(a));
    a.n = stream_bytes; a.index = d_index; a.n_nals = n_nals; a.keep = d_keep;
    a.nal_au = d_nal_au; a.n_aus = n_aus; a.sample_off = d_nal_au ? reinterpret_cast<unsigned long long*>(d_sample_off) : nullptr;
    a.out_cap = out_cap; a.index_out = d_index_out; a.summary = d_summary;
    a.t.src = d_stream; a.t.out = d_out; a.t.prefix = (uint32_t)length_size; a.t.prefix_is_length = 1;
    const uint64_t most = stream_bytes + n_nals * (uint64_t)length_size;                    /* the output is at most this long */
    a.t.tiles = d_out ? hbs::piece_tiles(out_cap < most ? out_cap : most) : 0;
    return carve_and_launch(c, c->buf[kLws], "hipMalloc(lenpref scratch)", a, hbs::lay_a2l, hbs::launch_annexb_to_lenpref, "launch_annexb_to_lenpref");
}

int hbs_lenpref_to_annexb(hbs_ctx* c, const uint8_t* d_in, uint64_t in_bytes, int length_size,
                          const uint64_t* d_sample_off, const uint64_t* d_sample_size, uint64_t n_samples,
                          int startcode_bytes, uint64_t nal_cap, uint8_t* d_out, uint64_t out_cap,
                          uint64_t* d_sample_off_out, hbs_summary* d_summary)
{
    if (!c || !d_summary || (length_size != 1 && length_size != 2 && length_size != 4) ||
        (startcode_bytes != 3 && startcode_bytes != 4)) return HBS_E_ARG;
    if (n_samples && (!d_sample_off || !d_sample_size || (in_bytes && !d_in))) return HBS_E_ARG;
    if (misaligned_refused(c, "input/output/summary pointers must be 16-byte aligned, sample tables 8-byte aligned",
                           {d_in, d_out, d_summary}, {d_sample_off, d_sample_size, d_sample_off_out})) return HBS_E_ARG;
    if (out_cap_refused(c, d_out, out_cap)) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::L2aArgs a;
    memset(&a, 0, sizeof(a));
    a.n = in_bytes; a.length_size = (uint32_t)length_size;
    a.sample_off = reinterpret_cast<const unsigned long long*>(d_sample_off);
    a.sample_size = reinterpret_cast<const unsigned long long*>(d_sample_size); a.n_samples = n_samples;
    /* what sizes the piece table: a record is at least its start code in the output, so more than out_cap / startcode_bytes
     * records do not fit out_cap either (HBS_E_CAPACITY) and the place kernel never sees them */
    const uint64_t fit = out_cap / (uint64_t)startcode_bytes;
    a.nal_cap = nal_cap; a.piece_cap = d_out ? (nal_cap < fit ? nal_cap : fit) : 0; a.out_cap = out_cap;
    a.sample_off_out = reinterpret_cast<unsigned long long*>(d_sample_off_out); a.summary = d_summary;
    a.t.src = d_in; a.t.out = d_out; a.t.prefix = (uint32_t)startcode_bytes; a.t.prefix_is_length = 0;
    a.t.tiles = d_out ? hbs::piece_tiles(out_cap) : 0;              /* (samples may overlap: the input's size bounds nothing; out_cap is bounded above) */
    return carve_and_launch(c, c->buf[kLws], "hipMalloc(lenpref scratch)", a, hbs::lay_l2a, hbs::launch_lenpref_to_annexb, "launch_lenpref_to_annexb");
}

int hbs_ts_demux(hbs_ctx* c, const uint8_t* d_ts, uint64_t ts_bytes, int packet_bytes, int pid,
                 uint8_t* d_out, uint64_t out_cap, hbs_ts_pes* d_pes, uint64_t pes_cap, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_ts_pes) == 32 && sizeof(hbs_ts_packet) == 48, "hbs_ts_pes / hbs_ts_packet layout");
    if (!c || !d_summary || !hbs::ts_packet_bytes_ok(packet_bytes) || pid < 0 || pid > 8191) return HBS_E_ARG;
    if (ts_bytes % (uint64_t)packet_bytes || ts_bytes / (uint64_t)packet_bytes > 0xFFFFFFFFull || (ts_bytes && !d_ts)) return HBS_E_ARG;
    if (misaligned_refused(c, "transport stream/output/summary pointers must be 16-byte aligned, the PES table 8-byte aligned",
                           {d_ts, d_out, d_summary}, {d_pes})) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::TsArgs a;
    memset(&a, 0, sizeof(a));
    a.ts = d_ts; a.n = ts_bytes; a.packets = ts_bytes / (uint64_t)packet_bytes;
    a.B = (uint32_t)packet_bytes; a.lead = hbs::ts_lead(packet_bytes); a.pid = pid;
    a.out = d_out; a.out_cap = out_cap; a.pes = d_pes; a.pes_cap = pes_cap; a.summary = d_summary;
    return carve_and_launch(c, c->buf[kTws], "hipMalloc(transport stream scratch)", a, hbs::lay_ts, hbs::launch_ts_demux, "launch_ts_demux");
}

int hbs_ts_mux(hbs_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes,
               const hbs_access_unit* d_au, uint64_t n_aus, const uint64_t* d_pts, const uint64_t* d_dts,
               const hbs_ts_mux_params* params, uint8_t* d_out, uint64_t out_cap, uint32_t* d_au_packet, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_ts_mux_params) == 48 && sizeof(hbs_access_unit) == 64, "hbs_ts_mux_params / hbs_access_unit layout");
    if (!c || !d_summary || !hbs::tsm_params_ok(params) || n_aus > 0xFFFFFFFFull) return HBS_E_ARG;
    if (n_aus && (!d_au || (stream_bytes && !d_stream))) return HBS_E_ARG;
    if (misaligned_refused(c, "stream/output/AU table/summary pointers must be 16-byte aligned, the times 8-byte, the packet numbers 4-byte",
                           {d_stream, d_out, d_au, d_summary}, {d_pts, d_dts}, {d_au_packet})) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::TsmArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_stream; a.n = stream_bytes; a.au = d_au; a.n_aus = n_aus;
    a.pts = reinterpret_cast<const unsigned long long*>(d_pts); a.dts = reinterpret_cast<const unsigned long long*>(d_dts);
    a.B = (uint32_t)params->packet_bytes; a.lead = hbs::ts_lead(params->packet_bytes); a.pid = (uint32_t)params->pid;
    a.flags = params->flags; a.cc_es = params->cc_es; a.cc_pat = params->cc_pat; a.cc_pmt = params->cc_pmt; a.pcr_lead = params->pcr_lead;
    a.out = d_out; a.out_cap = out_cap; a.au_packet = d_out ? d_au_packet : nullptr; a.summary = d_summary;
    uint8_t psi[2][188];
    if (hbs::tsm_psi_host(params, psi[0], psi[1]) != 0) return HBS_E_ARG;
    memcpy(&a.psi, psi, sizeof(a.psi));
    /* the copy's grid: the packets out_cap has room for, and no more than the call can make */
    const uint64_t fit = out_cap / a.B, most = hbs::tsm_packet_bound(n_aus, stream_bytes);
    const uint64_t reach = d_out && n_aus ? (fit < most ? fit : most) : 0;
    a.copy_blocks = (reach + hbs::kTsmPacketsPerBlock - 1) / hbs::kTsmPacketsPerBlock;
    return carve_and_launch(c, c->buf[kMws], "hipMalloc(transport mux scratch)", a, hbs::lay_tsm, hbs::launch_ts_mux, "launch_ts_mux");
}

int hbs_rtp_pack(hbs_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes,
                 const hbs_nal_entry* d_index, uint64_t n_nals, const uint32_t* d_nal_au, uint64_t n_aus, const uint64_t* d_pts,
                 const hbs_rtp_params* params, uint8_t* d_out, uint64_t out_cap,
                 uint64_t* d_nal_off, uint64_t* d_nal_packet, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_rtp_params) == 32 && sizeof(hbs_rtp_packet) == 72 && sizeof(hbs_nal_entry) == 32, "hbs_rtp_params / hbs_rtp_packet layout");
    if (!c || !d_summary || !hbs::rtp_params_ok(params) || n_nals > 0xFFFFFFFFull) return HBS_E_ARG;
    if (n_nals && (!d_index || !d_stream)) return HBS_E_ARG;
    if (misaligned_refused(c, "stream/output/summary pointers must be 16-byte aligned, index, times and the two tables 8-byte, AU numbers 4-byte",
                           {d_stream, d_out, d_summary}, {d_index, d_pts, d_nal_off, d_nal_packet}, {d_nal_au})) return HBS_E_ARG;
    if (out_cap_refused(c, d_out, out_cap)) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::RtpArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_stream; a.n = stream_bytes; a.index = d_index; a.n_nals = n_nals;
    a.nal_au = d_nal_au; a.n_aus = n_aus; a.pts = reinterpret_cast<const unsigned long long*>(d_pts);
    a.q = hbs::rtp_rule(params); a.flags = params->flags; a.ts_base = params->ts_base; a.ts_step = params->ts_step;
    a.out = d_out; a.out_cap = out_cap; a.summary = d_summary;
    if (d_out) { a.nal_off = reinterpret_cast<unsigned long long*>(d_nal_off); a.nal_packet = reinterpret_cast<unsigned long long*>(d_nal_packet); }
    /* the copy's grid: the tiles out_cap has room for, and no more than the call can make */
    const uint64_t most = hbs::rtp_output_bound(n_nals, stream_bytes, a.q);
    a.tiles = d_out && n_nals ? hbs::rtp_tiles(out_cap < most ? out_cap : most) : 0;
    return carve_and_launch(c, c->buf[kRws], "hipMalloc(RTP scratch)", a, hbs::lay_rtp, hbs::launch_rtp_pack, "launch_rtp_pack");
}

int hbs_rtp_unpack(hbs_ctx* c, const uint8_t* d_in, uint64_t in_bytes,
                   const uint64_t* d_pkt_off, const uint64_t* d_pkt_size, uint64_t n_packets,
                   const hbs_rtp_unpack_params* params, uint8_t* d_out, uint64_t out_cap,
                   hbs_nal_entry* d_index_out, uint32_t* d_nal_au_out, uint64_t nal_cap,
                   uint64_t* d_au_ts_out, uint64_t au_cap, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_rtp_unpack_params) == 16, "hbs_rtp_unpack_params layout");
    if (!c || !d_summary || !hbs::rtpu_params_ok(params) || n_packets > 0xFFFFFFFFull) return HBS_E_ARG;
    if (n_packets && (!d_pkt_off || !d_pkt_size || (in_bytes && !d_in))) return HBS_E_ARG;
    if (misaligned_refused(c, "input/output/summary pointers must be 16-byte aligned, packet tables, output index and AU times 8-byte, AU numbers 4-byte",
                           {d_in, d_out, d_summary}, {d_pkt_off, d_pkt_size, d_index_out, d_au_ts_out}, {d_nal_au_out})) return HBS_E_ARG;
    if (out_cap_refused(c, d_out, out_cap)) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::RtpuArgs a;
    memset(&a, 0, sizeof(a));
    a.n = in_bytes;
    a.pkt_off = reinterpret_cast<const unsigned long long*>(d_pkt_off);
    a.pkt_size = reinterpret_cast<const unsigned long long*>(d_pkt_size); a.n_packets = n_packets;
    a.q = hbs::rtpu_rule(params);
    a.out_cap = out_cap; a.nal_cap = nal_cap; a.au_cap = au_cap; a.summary = d_summary;
    if (d_out) { a.index_out = d_index_out; a.nal_au_out = d_nal_au_out; a.au_ts_out = reinterpret_cast<unsigned long long*>(d_au_ts_out); }
    a.t.src = d_in; a.t.out = d_out;
    a.t.tiles = d_out ? hbs::piece_tiles(out_cap) : 0;              /* (packets may overlap: the input's size bounds nothing; out_cap is bounded above) */
    return carve_and_launch(c, c->buf[kUws], "hipMalloc(RTP unpack scratch)", a, hbs::lay_rtpu, hbs::launch_rtp_unpack, "launch_rtp_unpack");
}

int hbs_rtp_order(hbs_ctx* c, const uint8_t* d_in, uint64_t in_bytes,
                  const uint64_t* d_pkt_off, const uint64_t* d_pkt_size, uint64_t n_packets,
                  const hbs_rtp_order_params* params, uint64_t* d_off_out, uint64_t* d_size_out,
                  uint32_t* d_src_out, uint64_t* d_ext_out, uint64_t out_cap, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_rtp_order_params) == 32, "hbs_rtp_order_params layout");
    if (!c || !d_summary || !hbs::rtpo_params_ok(params) || n_packets > hbs::kRtpoMaxPackets) return HBS_E_ARG;
    if (n_packets && (!d_pkt_off || !d_pkt_size || (in_bytes && !d_in))) return HBS_E_ARG;
    if ((d_off_out == nullptr) != (d_size_out == nullptr) || (!d_off_out && (d_src_out || d_ext_out))) return HBS_E_ARG;
    if (misaligned_refused(c, "input/summary pointers must be 16-byte aligned, packet tables and 64-bit output tables 8-byte, table positions 4-byte",
                           {d_in, d_summary}, {d_pkt_off, d_pkt_size, d_off_out, d_size_out, d_ext_out}, {d_src_out})) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::RtpoArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_in; a.n = in_bytes;
    a.pkt_off = reinterpret_cast<const unsigned long long*>(d_pkt_off);
    a.pkt_size = reinterpret_cast<const unsigned long long*>(d_pkt_size); a.n_packets = n_packets;
    a.q = hbs::rtpo_rule(params);
    a.off_out = reinterpret_cast<unsigned long long*>(d_off_out); a.size_out = reinterpret_cast<unsigned long long*>(d_size_out);
    a.src_out = d_src_out; a.ext_out = reinterpret_cast<unsigned long long*>(d_ext_out);
    a.out_cap = out_cap; a.summary = d_summary;
    return carve_and_launch(c, c->buf[kOws], "hipMalloc(RTP order scratch)", a, hbs::lay_rtpo, hbs::launch_rtp_order, "launch_rtp_order");
}

int hbs_mp4_fragment(hbs_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes,
                     const hbs_nal_entry* d_index, uint64_t n_nals, const uint8_t* d_keep,
                     const uint32_t* d_nal_au, const hbs_access_unit* d_au, uint64_t n_aus,
                     const uint64_t* d_dts, const uint64_t* d_pts, const hbs_mp4_params* params,
                     uint8_t* d_out, uint64_t out_cap, uint64_t* d_sample_off, uint64_t* d_sample_size,
                     hbs_mp4_frag* d_frag, uint64_t frag_cap, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_mp4_params) == 32 && sizeof(hbs_mp4_frag) == 48 && sizeof(hbs_mp4_init_params) == 32, "hbs_mp4_* layout");
    if (!c || !d_summary || !hbs::mp4_params_ok(params) || n_nals > 0xFFFFFFFFull || n_aus > 0xFFFFFFFFull) return HBS_E_ARG;
    if (n_nals ? (!d_index || !d_nal_au || (stream_bytes && !d_stream)) : n_aus != 0) return HBS_E_ARG;
    if (n_aus && !d_au) return HBS_E_ARG;
    if ((d_sample_off == nullptr) != (d_sample_size == nullptr)) return HBS_E_ARG;
    if (misaligned_refused(c, "stream/output/AU table/fragment table/summary pointers must be 16-byte aligned, index, times and sample tables 8-byte, AU numbers 4-byte",
                           {d_stream, d_out, d_au, d_frag, d_summary}, {d_index, d_dts, d_pts, d_sample_off, d_sample_size}, {d_nal_au})) return HBS_E_ARG;
    if (out_cap_refused(c, d_out, out_cap)) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::Mp4Args a;
    memset(&a, 0, sizeof(a));
    a.src = d_stream; a.n = stream_bytes; a.index = d_index; a.n_nals = n_nals; a.keep = d_keep;
    a.nal_au = d_nal_au; a.au = d_au; a.n_aus = n_aus;
    a.dts = reinterpret_cast<const unsigned long long*>(d_dts); a.pts = reinterpret_cast<const unsigned long long*>(d_pts);
    a.L = (uint32_t)params->length_size; a.flags = params->flags; a.track_id = params->track_id; a.sequence = params->sequence;
    a.max_samples = params->max_samples; a.sample_duration = params->sample_duration; a.base_time = params->base_time;
    a.out = d_out; a.out_cap = out_cap; a.summary = d_summary;
    if (d_out) {
        a.sample_off = reinterpret_cast<unsigned long long*>(d_sample_off); a.sample_size = reinterpret_cast<unsigned long long*>(d_sample_size);
        a.frag = d_frag; a.frag_cap = frag_cap;
    }
    /* the copy's grid: the tiles out_cap has room for, and no more than the call can make */
    const uint64_t most = hbs::mp4_output_bound(n_nals, n_aus, stream_bytes, a.L);
    a.tiles = d_out && n_nals ? hbs::mp4_tiles(out_cap < most ? out_cap : most) : 0;
    return carve_and_launch(c, c->buf[kPws], "hipMalloc(MP4 scratch)", a, hbs::lay_mp4, hbs::launch_mp4_fragment, "launch_mp4_fragment");
}

int hbs_mp4_protect(hbs_ctx* c, const uint8_t* d_in, uint64_t in_bytes, const hbs_mp4_frag* d_frag, uint64_t n_frags,
                    const uint64_t* d_sub_first, const hbs_cenc_subsample* d_sub, const uint8_t* d_iv, uint64_t n_samples,
                    const hbs_mp4_protect_params* params, uint8_t* d_out, uint64_t out_cap,
                    uint64_t* d_sample_off, uint64_t* d_sample_size, hbs_mp4_frag* d_frag_out, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_mp4_protect_params) == 32 && sizeof(hbs_mp4_tenc) == 64, "hbs_mp4_protect layouts");
    if (!c || !d_summary || !hbs::mp4_protect_params_ok(params) || n_frags > 0xFFFFFFFFull || n_samples > 0xFFFFFFFFull) return HBS_E_ARG;
    if (n_frags ? (!d_frag || (in_bytes && !d_in)) : n_samples != 0) return HBS_E_ARG;
    if (n_samples && (!d_sub_first || !d_sub || (params->iv_size && !d_iv))) return HBS_E_ARG;
    if ((d_sample_off == nullptr) != (d_sample_size == nullptr)) return HBS_E_ARG;
    if (misaligned_refused(c, "input/output/fragment tables/IV/summary pointers must be 16-byte aligned, the 64-bit tables and the entries 8-byte",
                           {d_in, d_out, d_frag, d_frag_out, d_iv, d_summary}, {d_sub_first, d_sub, d_sample_off, d_sample_size})) return HBS_E_ARG;
    if (out_cap_refused(c, d_out, out_cap)) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::Mp4ProtArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_in; a.n = in_bytes; a.frag = d_frag; a.n_frags = n_frags;
    a.sub_first = reinterpret_cast<const unsigned long long*>(d_sub_first); a.sub = d_sub; a.iv = d_iv; a.n_samples = n_samples;
    a.V = params->iv_size; a.out = d_out; a.out_cap = out_cap; a.summary = d_summary;
    if (d_out) {
        a.sample_off = reinterpret_cast<unsigned long long*>(d_sample_off); a.sample_size = reinterpret_cast<unsigned long long*>(d_sample_size);
        a.frag_out = d_frag_out;
        a.tiles = n_frags ? hbs::mp4prot_tiles(out_cap) : 0;                 /* the copy's grid: the tiles out_cap has room for */
    }
    return carve_and_launch(c, c->buf[kEws], "hipMalloc(MP4 protect scratch)", a, hbs::lay_mp4prot, hbs::launch_mp4_protect, "launch_mp4_protect");
}

int hbs_mp4_senc_samples(hbs_ctx* c, const uint8_t* d_in, uint64_t in_bytes, const hbs_mp4_frag* d_frag, uint64_t n_frags,
                         const uint64_t* d_sample_size, uint64_t n_samples, const hbs_mp4_senc_params* params,
                         uint64_t* d_sub_first, hbs_cenc_subsample* d_sub, uint64_t sub_cap, uint8_t* d_iv, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_mp4_senc_params) == 32 && sizeof(hbs::SencFind) == 40, "hbs_mp4_senc_samples layouts");
    if (!c || !d_summary || !d_sub_first || !hbs::mp4_senc_params_ok(params)) return HBS_E_ARG;
    if (n_frags > 0xFFFFFFFFull || n_samples > 0xFFFFFFFFull || in_bytes > hbs::kRdMaxIn) return HBS_E_ARG;
    if (n_frags ? (!d_frag || (in_bytes && !d_in)) : n_samples != 0) return HBS_E_ARG;
    if (n_samples && params->iv_size && !d_iv) return HBS_E_ARG;
    if (misaligned_refused(c, "input/fragment table/IV/summary pointers must be 16-byte aligned, the sample sizes and the two subsample tables 8-byte",
                           {d_in, d_frag, d_iv, d_summary}, {d_sample_size, d_sub_first, d_sub})) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::Mp4SencArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_in; a.n = in_bytes; a.frag = d_frag; a.n_frags = n_frags;
    a.sample_size = reinterpret_cast<const unsigned long long*>(d_sample_size); a.n_samples = n_samples;
    a.V = params->iv_size; a.track_id = params->track_id; a.flags = params->flags;
    a.sub_first = reinterpret_cast<unsigned long long*>(d_sub_first); a.sub = d_sub; a.sub_cap = sub_cap; a.iv = d_iv; a.summary = d_summary;
    return carve_and_launch(c, c->buf[kNws], "hipMalloc(MP4 senc scratch)", a, hbs::lay_mp4senc, hbs::launch_mp4_senc_samples, "launch_mp4_senc_samples");
}

int hbs_mp4_samples(hbs_ctx* c, const uint8_t* d_in, uint64_t in_bytes, const void* d_seg, uint64_t seg_stride, uint64_t n_segs,
                    const hbs_mp4_read_params* params, uint64_t moof_cap, uint64_t sample_cap,
                    uint64_t* d_sample_off, uint64_t* d_sample_size, uint64_t* d_dts, uint64_t* d_pts, uint32_t* d_sample_flags,
                    hbs_mp4_frag* d_frag, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_mp4_read_params) == 32 && sizeof(hbs_mp4_track) == 64 && sizeof(hbs::Mp4TrunRec) == 64, "hbs_mp4_samples layouts");
    if (!c || !d_summary || !hbs::mp4_read_params_ok(params) || in_bytes > hbs::kRdMaxIn || (in_bytes && !d_in)) return HBS_E_ARG;
    if (d_seg && (seg_stride < 16 || seg_stride % 8 != 0 || n_segs > 0xFFFFFFFFull)) return HBS_E_ARG;
    if ((d_sample_off == nullptr) != (d_sample_size == nullptr)) return HBS_E_ARG;
    if (!d_sample_off && (d_dts || d_pts || d_sample_flags || d_frag)) return HBS_E_ARG;
    if (moof_cap > 0xFFFFFFFFull || (d_sample_off && sample_cap > 0xFFFFFFFFull)) return HBS_E_ARG;
    if (misaligned_refused(c, "input/fragment table/summary pointers must be 16-byte aligned, segment table and 64-bit sample tables 8-byte, sample flags 4-byte",
                           {d_in, d_frag, d_summary}, {d_seg, d_sample_off, d_sample_size, d_dts, d_pts}, {d_sample_flags})) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::Mp4RdArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_in; a.n = in_bytes;
    a.seg = static_cast<const uint8_t*>(d_seg); a.seg_stride = seg_stride; a.n_segs = d_seg ? n_segs : 1;
    a.x.track_id = params->track_id; a.x.dur = params->trex_duration; a.x.size = params->trex_size; a.x.flags = params->trex_flags;
    a.moof_cap = moof_cap; a.summary = d_summary;
    if (d_sample_off) {
        a.out = true; a.sample_cap = sample_cap;
        a.sample_off = reinterpret_cast<unsigned long long*>(d_sample_off); a.sample_size = reinterpret_cast<unsigned long long*>(d_sample_size);
        a.dts = reinterpret_cast<unsigned long long*>(d_dts); a.pts = reinterpret_cast<unsigned long long*>(d_pts);
        a.sample_flags = d_sample_flags; a.frag = d_frag;
    }
    return carve_and_launch(c, c->buf[kQws], "hipMalloc(MP4 read scratch)", a, hbs::lay_mp4rd, hbs::launch_mp4_samples, "launch_mp4_samples");
}

int hbs_mp4_stbl_samples(hbs_ctx* c, const uint8_t* d_in, uint64_t in_bytes, const hbs_mp4_stbl* tables, uint64_t sample_cap,
                         uint64_t* d_sample_off, uint64_t* d_sample_size, uint64_t* d_dts, uint64_t* d_pts, uint32_t* d_sample_flags,
                         hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_mp4_stbl) == 128 && sizeof(hbs_mp4_box_ref) == 16, "hbs_mp4_stbl_samples layouts");
    if (!c || !d_summary || !d_in || !hbs::mp4_stbl_ok(tables) || in_bytes > hbs::kRdMaxIn || tables->file_bytes > hbs::kRdMaxIn) return HBS_E_ARG;
    if ((d_sample_off == nullptr) != (d_sample_size == nullptr)) return HBS_E_ARG;
    if (!d_sample_off && (d_dts || d_pts || d_sample_flags)) return HBS_E_ARG;
    if (d_sample_off && sample_cap > 0xFFFFFFFFull) return HBS_E_ARG;
    if (misaligned_refused(c, "input/summary pointers must be 16-byte aligned, the 64-bit sample tables 8-byte, sample flags 4-byte",
                           {d_in, d_summary}, {d_sample_off, d_sample_size, d_dts, d_pts}, {d_sample_flags})) return HBS_E_ARG;
    hbs::StblArgs a;
    memset(&a, 0, sizeof(a));
    const hbs_mp4_box_ref* ref[hbs::kStBoxes] = {&tables->stsz, &tables->stco, &tables->stsc, &tables->stts, &tables->ctts, &tables->stss};
    a.co64 = (tables->flags & HBS_MP4_STBL_CO64) != 0u;
    const uint64_t fixed[hbs::kStBoxes] = {12, 8, 8, 8, 8, 8}, entry[hbs::kStBoxes] = {4, a.co64 ? 8u : 4u, 12, 8, 8, 4};
    for (int b = 0; b < hbs::kStBoxes; ++b) {
        const uint64_t off = ref[b]->off, bytes = ref[b]->bytes;
        if (!bytes && b <= hbs::kStts) { snprintf(c->err, sizeof(c->err), "stsz, stco / co64, stsc and stts are required"); return HBS_E_ARG; }
        if (bytes && (off > in_bytes || bytes > in_bytes - off)) { snprintf(c->err, sizeof(c->err), "a table box leaves the buffer"); return HBS_E_ARG; }
        a.box[b].off = bytes ? off : 0; a.box[b].bytes = bytes;
        /* what sizes the grids and the scratch: the entries the payload has bytes for (a count has 32 bits) */
        const uint64_t room = bytes > fixed[b] ? (bytes - fixed[b]) / entry[b] : 0;
        a.cap[b] = room < 0xFFFFFFFFull ? room : 0xFFFFFFFFull;
    }
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    a.src = d_in; a.n = in_bytes; a.file_bytes = tables->file_bytes ? tables->file_bytes : in_bytes;
    a.summary = d_summary;
    if (d_sample_off) {
        a.out = true; a.sample_cap = sample_cap;
        a.sample_off = reinterpret_cast<unsigned long long*>(d_sample_off); a.sample_size = reinterpret_cast<unsigned long long*>(d_sample_size);
        a.dts = reinterpret_cast<unsigned long long*>(d_dts); a.pts = reinterpret_cast<unsigned long long*>(d_pts);
        a.sample_flags = d_sample_flags;
    }
    return carve_and_launch(c, c->buf[kSws], "hipMalloc(MP4 sample table scratch)", a, hbs::lay_mp4stbl, hbs::launch_mp4_stbl_samples, "launch_mp4_stbl_samples");
}

int hbs_mp4_stbl_write(hbs_ctx* c, const uint64_t* d_sample_off, const uint64_t* d_sample_size, uint64_t n_samples, const uint64_t* d_dts,
                       const uint64_t* d_pts, const uint32_t* d_sample_flags, const hbs_mp4_stbl_write_params* params, uint8_t* d_out,
                       uint64_t out_cap, hbs_mp4_stbl* d_tables, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_mp4_stbl_write_params) == 32, "hbs_mp4_stbl_write_params layout");
    if (!c || !d_summary || !hbs::mp4_stbl_write_params_ok(params) || n_samples > 0xFFFFFFFFull) return HBS_E_ARG;
    if (n_samples && (!d_sample_off || !d_sample_size)) return HBS_E_ARG;
    if (misaligned_refused(c, "output/box record/summary pointers must be 16-byte aligned, the 64-bit sample tables 8-byte, sample flags 4-byte",
                           {d_out, d_tables, d_summary}, {d_sample_off, d_sample_size, d_dts, d_pts}, {d_sample_flags})) return HBS_E_ARG;
    if (out_cap_refused(c, d_out, out_cap)) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::StblwArgs a;
    memset(&a, 0, sizeof(a));
    a.in.off = d_sample_off; a.in.size = d_sample_size; a.in.n = n_samples; a.in.dts = d_dts; a.in.pts = d_pts; a.in.sflags = d_sample_flags;
    a.in.sample_duration = params->sample_duration; a.in.base_time = params->base_time; a.in.data_offset = params->data_offset;
    a.co64 = (params->flags & HBS_MP4_STBL_CO64) != 0u; a.max_chunk = params->max_chunk_samples;
    a.out = d_out; a.out_cap = out_cap; a.tables = d_tables; a.summary = d_summary;
    return carve_and_launch(c, c->buf[kVws], "hipMalloc(MP4 sample table writer scratch)", a, hbs::lay_mp4stblw, hbs::launch_mp4_stbl_write, "launch_mp4_stbl_write");
}

int hbs_au_insert(hbs_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes,
                  const hbs_nal_entry* d_index, const hbs_parsed_nal* d_parsed, uint64_t n_nals,
                  const hbs_access_unit* d_au, const uint32_t* d_nal_au, uint64_t n_aus,
                  uint64_t first_au, uint64_t au_count, uint32_t flags, uint8_t* d_out, uint64_t out_cap,
                  hbs_nal_entry* d_index_out, uint32_t* d_nal_src, uint32_t* d_nal_au_out, uint64_t index_cap,
                  hbs_access_unit* d_au_out, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_access_unit) == 64 && sizeof(hbs_parsed_nal) == 32 && sizeof(hbs_nal_entry) == 32, "record layouts");
    if (!c || !d_summary || (flags & ~hbs::kAuinsFlags) || n_nals > 0xFFFFFFFFull || n_aus > 0xFFFFFFFFull) return HBS_E_ARG;
    if (n_nals && (!d_index || !d_parsed || (stream_bytes && !d_stream))) return HBS_E_ARG;
    if (n_aus && (!d_au || (n_nals && !d_nal_au))) return HBS_E_ARG;
    if (misaligned_refused(c, "stream/output/index/parsed/AU table/summary pointers must be 16-byte aligned, the output index 8-byte, the per-NAL numbers 4-byte",
                           {d_stream, d_out, d_index, d_parsed, d_au, d_au_out, d_summary}, {d_index_out}, {d_nal_au, d_nal_src, d_nal_au_out})) return HBS_E_ARG;
    if (out_cap_refused(c, d_out, out_cap)) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::AuinsArgs a;
    memset(&a, 0, sizeof(a));
    a.n = stream_bytes; a.index = d_index; a.parsed = d_parsed; a.n_nals = n_nals;
    a.au = d_au; a.nal_au = d_nal_au; a.n_aus = n_aus;
    a.a0 = first_au < n_aus ? first_au : 0;                         /* the range, clipped as hbs_au_keep clips it */
    a.cnt = first_au < n_aus ? (au_count < n_aus - first_au ? au_count : n_aus - first_au) : 0;
    if (!n_nals) a.cnt = 0;
    a.flags = flags; a.out_cap = out_cap; a.index_cap = index_cap; a.summary = d_summary;
    if (d_out) { a.index_out = d_index_out; a.nal_src = d_nal_src; a.nal_au_out = d_nal_au_out; a.au_out = d_au_out; }
    a.t.src = d_stream; a.t.out = d_out; a.t.tiles = d_out && a.cnt ? hbs::piece_tiles(out_cap) : 0;
    return carve_and_launch(c, c->buf[kIws], "hipMalloc(AU insert scratch)", a, hbs::lay_auins, hbs::launch_au_insert, "launch_au_insert");
}

int hbs_aud_nal_host(int temporal_id_plus1, uint32_t slice_types, uint8_t out[7]) { return hbs::auins_aud_host(temporal_id_plus1, slice_types, out); }

uint64_t hbs_au_sps_poc_offset(void) { return offsetof(hevc_sps_t, log2_max_pic_order_cnt_lsb_minus4); }

int hbs_access_units(hbs_ctx* c, const hbs_nal_entry* d_index, const hbs_parsed_nal* d_parsed,
                     const hbs_slice_compact* d_compact, const uint8_t* d_structs, uint64_t n_nals,
                     const hbs_au_carry* initial, hbs_access_unit* d_au, uint64_t au_cap, uint32_t* d_nal_au,
                     hbs_au_carry* d_carry_out, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_access_unit) == 64 && sizeof(hbs_au_carry) == 16, "hbs_access_unit / hbs_au_carry layout");
    static_assert(sizeof(hbs_parsed_nal) == 32 && sizeof(hbs_slice_compact) == 64 && sizeof(hbs_nal_entry) == 32, "record layouts");
    if (!c || !d_summary || n_nals > 0xFFFFFFFFull) return HBS_E_ARG;
    if (n_nals && (!d_index || !d_parsed || !d_compact)) return HBS_E_ARG;
    if (misaligned(d_index, 15) || misaligned(d_parsed, 15) || misaligned(d_compact, 15) || misaligned(d_au, 15) ||
        misaligned(d_nal_au, 3) || misaligned(d_carry_out, 3) || misaligned(d_structs, 3)) {
        snprintf(c->err, sizeof(c->err), "index / parsed / compact / au pointers must be 16-byte aligned");
        return HBS_E_ARG;
    }
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::AuArgs a;
    memset(&a, 0, sizeof(a));
    a.index = d_index; a.parsed = d_parsed; a.compact = d_compact; a.structs = d_structs;
    a.n_nals = n_nals; a.sps_off = hbs_au_sps_poc_offset();
    if (initial) a.initial = *initial;
    a.au = d_au; a.au_cap = au_cap; a.nal_au = d_au ? d_nal_au : nullptr; a.carry_out = d_carry_out; a.summary = d_summary;
    return carve_and_launch(c, c->buf[kAws], "hipMalloc(access unit scratch)", a, hbs::lay_access_units, hbs::launch_access_units, "launch_access_units");
}

int hbs_au_keep(hbs_ctx* c, const uint32_t* d_nal_au, const hbs_parsed_nal* d_parsed, uint64_t n_nals,
                uint64_t first_au, uint64_t au_count, int flags, uint8_t* d_keep)
{
    if (!c || n_nals > 0xFFFFFFFFull || (flags & ~HBS_AUKEEP_PARAM_SETS)) return HBS_E_ARG;
    if (n_nals && (!d_nal_au || !d_parsed || !d_keep)) return HBS_E_ARG;
    if (misaligned(d_nal_au, 3) || misaligned(d_parsed, 7)) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    const int rc = grow(c, c->buf[kAws], 256, "hipMalloc(access unit scratch)");
    if (rc < 0) return rc;
    hbs::AuKeepArgs a;
    a.nal_au = d_nal_au; a.parsed = d_parsed; a.n_nals = n_nals; a.first_au = first_au; a.au_count = au_count; a.flags = flags;
    a.keep = d_keep;
    a.sets = static_cast<uint32_t*>(c->buf[kAws].ptr);
    const hipError_t e = hbs::launch_au_keep(a, c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "launch_au_keep");
}

int hbs_au_times(hbs_ctx* c, const hbs_access_unit* d_au, uint64_t n_aus, const hbs_au_times_params* params,
                 uint64_t* d_dts, uint64_t* d_pts, uint32_t* d_order, uint32_t* d_display, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_au_times_params) == 32 && sizeof(hbs_access_unit) == 64, "hbs_au_times layouts");
    if (!c || !d_summary || !hbs::aut_params_ok(params, n_aus) || (n_aus && !d_au)) return HBS_E_ARG;
    if (misaligned_refused(c, "AU table/summary pointers must be 16-byte aligned, the times 8-byte, order and display 4-byte",
                           {d_au, d_summary}, {d_dts, d_pts}, {d_order, d_display})) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::AutArgs a;
    memset(&a, 0, sizeof(a));
    a.au = d_au; a.n = n_aus;
    a.flags = params->flags; a.tick = params->tick; a.base_time = params->base_time;
    a.delay_given = (params->flags & HBS_AUT_DELAY_GIVEN) ? params->delay : 0u;
    a.dts = reinterpret_cast<unsigned long long*>(d_dts); a.pts = reinterpret_cast<unsigned long long*>(d_pts);
    a.order = d_order; a.display = d_display; a.summary = d_summary;
    return carve_and_launch(c, c->buf[kXws], "hipMalloc(AU times scratch)", a, hbs::lay_au_times, hbs::launch_au_times, "launch_au_times");
}

int hbs_cenc_subsamples(hbs_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes,
                        const hbs_nal_entry* d_index, uint64_t n_nals, const uint8_t* d_keep,
                        const uint32_t* d_nal_au, uint64_t n_aus, const uint64_t* d_payload_off,
                        const hbs_cenc_plan_params* params,
                        uint64_t* d_sub_first, hbs_cenc_subsample* d_sub, uint64_t sub_cap, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_cenc_plan_params) == 16 && sizeof(hbs_cenc_subsample) == 8 && sizeof(hbs_cenc_params) == 48, "hbs_cenc_* layouts");
    if (!c || !d_summary || !d_sub_first || !hbs::cenc_plan_params_ok(params) || n_nals > 0xFFFFFFFFull || n_aus > 0xFFFFFFFFull) return HBS_E_ARG;
    if (n_nals ? (!d_index || !d_nal_au || (stream_bytes && !d_stream)) : n_aus != 0) return HBS_E_ARG;
    if (misaligned_refused(c, "stream/summary pointers must be 16-byte aligned, index, payload offsets and the two subsample tables 8-byte, AU numbers 4-byte",
                           {d_stream, d_summary}, {d_index, d_payload_off, d_sub_first, d_sub}, {d_nal_au})) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::CencPlanArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_stream; a.n = stream_bytes; a.index = d_index; a.n_nals = n_nals; a.keep = d_keep;
    a.nal_au = d_nal_au; a.n_aus = n_aus; a.payload_off = reinterpret_cast<const unsigned long long*>(d_payload_off);
    a.L = (uint32_t)params->length_size; a.flags = params->flags; a.clear_lead = params->clear_lead;
    a.sub_first = reinterpret_cast<unsigned long long*>(d_sub_first); a.sub = d_sub; a.sub_cap = sub_cap; a.summary = d_summary;
    return carve_and_launch(c, c->buf[kCws], "hipMalloc(CENC plan scratch)", a, hbs::lay_cenc_plan, hbs::launch_cenc_subsamples, "launch_cenc_subsamples");
}

int hbs_cenc_crypt(hbs_ctx* c, uint8_t* d_data, uint64_t data_bytes,
                   const uint64_t* d_sample_off, const uint64_t* d_sample_size, uint64_t n_samples,
                   const uint64_t* d_sub_first, const hbs_cenc_subsample* d_sub,
                   uint8_t* d_iv, const hbs_cenc_params* params, hbs_summary* d_summary)
{
    if (!c || !d_summary || !hbs::cenc_params_ok(params) || n_samples > 0xFFFFFFFFull || (data_bytes && !d_data)) return HBS_E_ARG;
    if (n_samples && (!d_sample_off || !d_sample_size || !d_sub_first || !d_sub || (params->iv_mode == 0 && !d_iv))) return HBS_E_ARG;
    if (misaligned_refused(c, "data/IV/summary pointers must be 16-byte aligned, sample and subsample tables 8-byte aligned",
                           {d_data, d_iv, d_summary}, {d_sample_off, d_sample_size, d_sub_first, d_sub})) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::CencCall a;
    memset(&a, 0, sizeof(a));
    a.data = d_data; a.n = data_bytes;
    a.sample_off = reinterpret_cast<const unsigned long long*>(d_sample_off);
    a.sample_size = reinterpret_cast<const unsigned long long*>(d_sample_size); a.n_samples = n_samples;
    a.sub_first = reinterpret_cast<const unsigned long long*>(d_sub_first); a.sub = d_sub;
    a.iv = d_iv; a.iv_mode = params->iv_mode; a.iv_base = hbs::cenc_be64(params->iv0); a.summary = d_summary;
    a.tiles = hbs::piece_tiles(data_bytes);            /* the protected bytes are no more than the data (kCencTileBytes is a piece tile) */
    static_assert(hbs::kCencTileBytes == hbs::kPieceTileBytes, "piece_tiles counts the crypt kernel's tiles");
    hbs::cenc_expand_key(params->key, a.key);          /* on the host; the round keys travel with the launch */
    const int rc = carve_and_launch(c, c->buf[kYws], "hipMalloc(CENC scratch)", a, hbs::lay_cenc, hbs::launch_cenc_crypt, "launch_cenc_crypt");
    memset(&a.key, 0, sizeof(a.key));
    return rc;
}

int hbs_cbcs_crypt(hbs_ctx* c, uint8_t* d_data, uint64_t data_bytes,
                   const uint64_t* d_sample_off, const uint64_t* d_sample_size, uint64_t n_samples,
                   const uint64_t* d_sub_first, const hbs_cenc_subsample* d_sub,
                   const uint8_t* d_iv, const hbs_cbcs_params* params, hbs_summary* d_summary)
{
    static_assert(sizeof(hbs_cbcs_params) == 48, "hbs_cbcs_params layout");
    if (!c || !d_summary || !hbs::cbcs_params_ok(params) || n_samples > 0xFFFFFFFFull || (data_bytes && !d_data)) return HBS_E_ARG;
    if (n_samples && (!d_sample_off || !d_sample_size || !d_sub_first || !d_sub || (params->iv_mode == 0 && !d_iv))) return HBS_E_ARG;
    if (misaligned_refused(c, "data/IV/summary pointers must be 16-byte aligned, sample and subsample tables 8-byte aligned",
                           {d_data, d_iv, d_summary}, {d_sample_off, d_sample_size, d_sub_first, d_sub})) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::CbcsCall a;
    memset(&a, 0, sizeof(a));
    a.data = d_data; a.n = data_bytes;
    a.sample_off = reinterpret_cast<const unsigned long long*>(d_sample_off);
    a.sample_size = reinterpret_cast<const unsigned long long*>(d_sample_size); a.n_samples = n_samples;
    a.sub_first = reinterpret_cast<const unsigned long long*>(d_sub_first); a.sub = d_sub;
    a.iv = const_cast<uint8_t*>(d_iv); a.iv_mode = params->iv_mode; a.summary = d_summary;      /* (only read) */
    a.pattern = hbs::cbcs_pattern(params->crypt_byte_block, params->skip_byte_block, params->flags);
    a.decrypt = (params->flags & HBS_CBCS_DECRYPT) ? 1u : 0u;
    hbs::cbcs_load_be(params->iv0, a.iv0);
    hbs::cenc_expand_key(params->key, a.ek);           /* on the host; the round keys travel with the launch */
    hbs::cbcs_expand_dec_key(a.ek, a.dk);
    const int rc = carve_and_launch(c, c->buf[kYws], "hipMalloc(CENC scratch)", a, hbs::lay_cbcs, hbs::launch_cbcs_crypt, "launch_cbcs_crypt");
    memset(&a.ek, 0, sizeof(a.ek)); memset(&a.dk, 0, sizeof(a.dk));
    return rc;
}

int hbs_synth_rbsp(hbs_ctx* c, uint64_t seed, uint64_t n_nals, int mode,
                   uint8_t* d_rbsp, uint64_t rbsp_cap, hbs_nal_entry* d_index, hbs_summary* d_summary)
{
    if (!c || !d_summary || (n_nals && (!d_rbsp || !d_index)) || (mode != 0 && mode != 1)) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hbs::SynthArgs a;
    a.seed = seed; a.n = n_nals; a.mode = mode; a.rbsp = d_rbsp; a.rbsp_cap = rbsp_cap; a.index = d_index; a.summary = d_summary;
    const int rc = carve(c, c->buf[kWs], "hipMalloc(workspace)", [&](hbs::Carver& w) { hbs::lay_synth(w, a); });
    if (rc < 0) return rc;
    hipError_t e = hbs::launch_synth_rbsp(a, c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "launch_synth_rbsp");
}

uint64_t hbs_sps_slot_bytes(void) { return hbs::slot_bytes_of(HEVC_NAL_UNIT_TYPE_SPS_NUT); }
uint64_t hbs_sps_tables_offset(void) { return hbs::round16(sizeof(hevc_sps_t)); }

uint64_t hbs_synth_rbsp_bound(uint64_t n_nals) { return n_nals * 12288ull + 16; }
uint64_t hbs_annexb_bound(uint64_t rbsp_bytes, uint64_t n_nals) { return rbsp_bytes + rbsp_bytes / 2 + 4 * n_nals + 16; }
/* gap_mode 0: the gaps are whatever the index says (a start code, plus any zero bytes that stood in front of it) */
uint64_t hbs_annexb_bound_gaps(uint64_t rbsp_bytes, uint64_t n_nals, uint64_t gap_bytes) { (void)n_nals; return rbsp_bytes + rbsp_bytes / 2 + gap_bytes + 16; }

int hbs_parse_headers(hbs_ctx* c, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                      hbs_parsed_nal* d_parsed, uint8_t* d_structs, uint64_t structs_cap, hbs_summary* d_summary)
{
    return hbs_parse_headers_ctx(c, d_rbsp, d_index, n_nals, d_parsed, d_structs, structs_cap, nullptr, nullptr, d_summary);
}

int hbs_parse_extended(hbs_ctx* c, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                       hbs_parsed_nal* d_parsed, hbs_ext_nal* d_ext)
{
    if (!c || (n_nals && (!d_rbsp || !d_index || !d_parsed || !d_ext))) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    static_assert(sizeof(hbs_parsed_nal) == sizeof(hbs::ParsedNal), "hbs_parsed_nal is hbs::ParsedNal");
    const hipError_t e = hbs::launch_parse_extended(d_rbsp, d_index, n_nals, reinterpret_cast<hbs::ParsedNal*>(d_parsed), d_ext, c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "hbs_parse_extended");
}

int hbs_parse_headers_ctx(hbs_ctx* c, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                          hbs_parsed_nal* d_parsed, uint8_t* d_structs, uint64_t structs_cap,
                          const uint8_t* d_initial_sps_slot, const uint8_t* d_initial_pps, hbs_summary* d_summary)
{
    return hbs_parse_headers_trace(c, d_rbsp, d_index, n_nals, d_parsed, d_structs, structs_cap, d_initial_sps_slot, d_initial_pps,
                                   nullptr, 0, nullptr, d_summary);
}

int hbs_parse_headers_trace(hbs_ctx* c, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                            hbs_parsed_nal* d_parsed, uint8_t* d_structs, uint64_t structs_cap,
                            const uint8_t* d_initial_sps_slot, const uint8_t* d_initial_pps,
                            hbs_trace_rec* d_trace, uint32_t trace_cap, uint32_t* d_trace_count, hbs_summary* d_summary)
{
    return hbs_parse_headers_state(c, d_rbsp, d_index, n_nals, d_parsed, d_structs, structs_cap, d_initial_sps_slot, d_initial_pps,
                                   d_trace, trace_cap, d_trace_count, d_summary, nullptr, nullptr);
}

int hbs_parse_headers_state(hbs_ctx* c, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                            hbs_parsed_nal* d_parsed, uint8_t* d_structs, uint64_t structs_cap,
                            const uint8_t* d_initial_sps_slot, const uint8_t* d_initial_pps,
                            hbs_trace_rec* d_trace, uint32_t trace_cap, uint32_t* d_trace_count, hbs_summary* d_summary,
                            uint8_t* d_state_sps_slot, uint8_t* d_state_pps)
{
    return parse_impl(c, d_rbsp, d_index, n_nals, d_parsed, d_structs, structs_cap, d_initial_sps_slot, d_initial_pps,
                      d_trace, trace_cap, d_trace_count, d_summary, d_state_sps_slot, d_state_pps, nullptr, nullptr, 0);
}

int hbs_parse_headers_compact(hbs_ctx* c, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                              hbs_parsed_nal* d_parsed, hbs_slice_compact* d_compact, uint8_t* d_structs, uint64_t structs_cap,
                              const uint8_t* d_initial_sps_slot, const uint8_t* d_initial_pps, hbs_summary* d_summary)
{
    if (!d_compact && n_nals) return HBS_E_ARG;
    return parse_impl(c, d_rbsp, d_index, n_nals, d_parsed, d_structs, structs_cap, d_initial_sps_slot, d_initial_pps,
                      nullptr, 0, nullptr, d_summary, nullptr, nullptr, d_compact, nullptr, 0);
}

int hbs_parse_materialize(hbs_ctx* c, const uint8_t* d_rbsp, const hbs_nal_entry* d_index, uint64_t n_nals,
                          hbs_parsed_nal* d_parsed, hbs_slice_compact* d_compact, uint8_t* d_structs, uint64_t structs_cap,
                          const uint8_t* d_initial_sps_slot, const uint8_t* d_initial_pps,
                          const uint64_t* d_nal_list, uint64_t n_list, hbs_summary* d_summary)
{
    if ((!d_compact && n_nals) || (n_list && !d_nal_list)) return HBS_E_ARG;
    return parse_impl(c, d_rbsp, d_index, n_nals, d_parsed, d_structs, structs_cap, d_initial_sps_slot, d_initial_pps,
                      nullptr, 0, nullptr, d_summary, nullptr, nullptr, d_compact, d_nal_list, n_list);
}

int hbs_index_parse(hbs_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes,
                    hbs_nal_entry* d_index, uint64_t index_cap, uint32_t header_window,
                    hbs_parsed_nal* d_parsed, uint8_t* d_structs, uint64_t structs_cap, uint64_t* d_payload_off,
                    hbs_summary* d_scan_summary, hbs_summary* d_parse_summary, uint64_t* nal_count_out)
{
    return index_parse_impl(c, d_stream, stream_bytes, d_index, index_cap, header_window, d_parsed, nullptr, d_structs, structs_cap, d_payload_off,
                            d_scan_summary, d_parse_summary, nal_count_out);
}

int hbs_index_parse_compact(hbs_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes,
                            hbs_nal_entry* d_index, uint64_t index_cap, uint32_t header_window,
                            hbs_parsed_nal* d_parsed, hbs_slice_compact* d_compact, uint8_t* d_structs, uint64_t structs_cap, uint64_t* d_payload_off,
                            hbs_summary* d_scan_summary, hbs_summary* d_parse_summary, uint64_t* nal_count_out)
{
    if (!d_compact) return HBS_E_ARG;
    return index_parse_impl(c, d_stream, stream_bytes, d_index, index_cap, header_window, d_parsed, d_compact, d_structs, structs_cap, d_payload_off,
                            d_scan_summary, d_parse_summary, nal_count_out);
}

int hbs_write_headers(hbs_ctx* c, const hbs_parsed_nal* d_parsed, uint64_t n_nals, uint8_t* d_structs,
                      const uint8_t* d_initial_sps_slot, const uint8_t* d_initial_pps,
                      uint8_t* d_rbsp_out, uint32_t rbsp_cap, hbs_written_nal* d_written)
{
    static_assert(sizeof(hbs_written_nal) == sizeof(hbs::WrittenNal), "public record == kernel record");
    if (!c || (n_nals && (!d_parsed || !d_structs || !d_rbsp_out || !d_written))) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    int rc = ensure_zeros(c);
    if (rc) return rc;
    hbs::WriteArgs a;
    a.parsed = reinterpret_cast<const hbs::ParsedNal*>(d_parsed); a.n = n_nals; a.structs = d_structs;
    a.rbsp_out = d_rbsp_out; a.rbsp_cap = rbsp_cap; a.written = reinterpret_cast<hbs::WrittenNal*>(d_written);
    a.zeros = static_cast<const uint8_t*>(c->buf[kZeros].ptr); a.initial_sps_slot = d_initial_sps_slot; a.initial_pps = d_initial_pps;
    rc = carve(c, c->buf[kWs], "hipMalloc(workspace)", [&](hbs::Carver& w) { (void)hbs::lay_headers_common(w, a); });
    if (rc < 0) return rc;
    hipError_t e = hbs::launch_write_headers(a, c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "launch_write_headers");
}

/* plain device-memory helpers so that C callers (hbs_legacy.c) need no HIP headers */
int hbs_dev_alloc(hbs_ctx* c, uint64_t bytes, void** out)
{
    if (!c || !out) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hipError_t e = hipMalloc(out, bytes ? bytes : 16);
    return e == hipSuccess ? 0 : fail(c, e, "hipMalloc");
}

int hbs_dev_free(hbs_ctx* c, void* p)
{
    if (!c) return HBS_E_ARG;
    (void)hipStreamSynchronize(c->stream);
    hipError_t e = hipFree(p);
    return e == hipSuccess ? 0 : fail(c, e, "hipFree");
}

int hbs_copy_to_device(hbs_ctx* c, void* d_dst, const void* h_src, uint64_t bytes)
{
    if (!c) return HBS_E_ARG;
    if (!bytes) return 0;
    hipError_t e = hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      /* the host buffer may be reused at once */
    return e == hipSuccess ? 0 : fail(c, e, "hipMemcpy(H2D)");
}

int hbs_copy_to_host(hbs_ctx* c, void* h_dst, const void* d_src, uint64_t bytes)
{
    if (!c) return HBS_E_ARG;
    if (!bytes) return 0;
    hipError_t e = hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "hipMemcpy(D2H)");
}

/* the same without the wait: h_src must be page-locked (hbs_host_alloc) and stay untouched until the stream
 * has passed the copy; the legacy wrappers use it to put a whole call behind ONE synchronisation */
int hbs_copy_to_device_async(hbs_ctx* c, void* d_dst, const void* h_src, uint64_t bytes)
{
    if (!c) return HBS_E_ARG;
    if (!bytes) return 0;
    hipError_t e = hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "hipMemcpyAsync(H2D)");
}

int hbs_copy_device(hbs_ctx* c, void* d_dst, const void* d_src, uint64_t bytes)
{
    if (!c) return HBS_E_ARG;
    if (!bytes) return 0;
    hipError_t e = hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "hipMemcpyAsync(D2D)");
}

int hbs_host_alloc(hbs_ctx* c, uint64_t bytes, void** out)
{
    if (!c || !out) return HBS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return HBS_E_NO_DEVICE;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault);
    return e == hipSuccess ? 0 : fail(c, e, "hipHostMalloc");
}

int hbs_host_free(hbs_ctx* c, void* p)
{
    if (!c) return HBS_E_ARG;
    if (!p) return 0;
    (void)hipStreamSynchronize(c->stream);
    hipError_t e = hipHostFree(p);
    return e == hipSuccess ? 0 : fail(c, e, "hipHostFree");
}

int hbs_fill_device(hbs_ctx* c, void* d_dst, int value, uint64_t bytes)
{
    if (!c) return HBS_E_ARG;
    if (!bytes) return 0;
    hipError_t e = hipMemsetAsync(d_dst, value, bytes, c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "hipMemsetAsync");
}

int hbs_read_summary(hbs_ctx* c, const hbs_summary* d_summary, hbs_summary* h_summary)
{
    if (!c || !d_summary || !h_summary) return HBS_E_ARG;
    hipError_t e = hipMemcpyAsync(h_summary, d_summary, sizeof(hbs_summary), hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return fail(c, e, "hipMemcpyAsync(summary)");
    e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? 0 : fail(c, e, "hipStreamSynchronize");
}

} // extern "C"

