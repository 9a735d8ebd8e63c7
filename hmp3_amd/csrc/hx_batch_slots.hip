// hx_batch_slots.hip - slot state: everything that saves, restores or restarts a stream of a batch (kernels: hx_slots.hip).
// A stream's checkpoint is its HxStream record and the three carried subband granules of each channel, of a converting batch
// the converter's state too; the blob that carries it is laid out in hx_types.h (HxStateHeader and the HX_STATE_OFF_* parts).
// With it a stream continues in another slot, another batch of the same configuration, another GPU or after a restart exactly
// where it stopped (the reference's equivalent is a copy of the CMp3Enc object).
// There is one implementation of each operation: a list of n slots, one launch.  The device-blob calls and
// hx_batch_reset_streams enqueue it like a plain device call: on the caller's stream, behind everything the batch has in
// flight (order_behind_submits: the deferred packing goes out ungated first), and without a host wait but the staging's.
// The host-blob calls wait for the work in flight, run it on the null stream through device staging and wait again; the
// single-slot calls are their n = 1 case.
#include <string>
#include "hx_rt.h"

static unsigned long long fnv1a(const void *d, size_t n, unsigned long long h = 1469598103934665603ull)
{
    const unsigned char *c = (const unsigned char *) d;
    for (size_t i = 0; i < n; i++) { h ^= c[i]; h *= 1099511628211ull; }
    return h;
}
// over the echoed control and the derived frame constants
static unsigned long long cfg_fingerprint(const HxParams &p)
{
    const int v[] = {p.totbitrate, p.samprate, p.h_mode, p.h_id, p.nchan, p.nsb_limit, p.band_limit, p.framebytes, p.main_framebytes, p.side_bytes,
                     p.ms_flag, p.hf_flag, p.vbr_flag, p.initialMNR, p.short_block_threshold};
    return fnv1a(v, sizeof(v), fnv1a(&p.ec, sizeof(p.ec)));
}
static unsigned long long plan_fingerprint(const HxSrcPlan &p) { return fnv1a(&p, sizeof(p)); }

extern "C" long long hx_batch_stream_state_bytes(const hx_batch *b) { return (long long) (b && b->nsrc ? HX_STATE_END_SRC : HX_STATE_END); }
extern "C" long long hx_batch_stream_states_stride(const hx_batch *b) { return b ? (hx_batch_stream_state_bytes(b) + 15) & ~15LL : 0; }

// what hx_batch_reset_stream[s] copies into a slot, and what a blob of each class carries
int slots_init(hx_batch *b)
{
    std::vector<HxStream> init(b->ncls);
    for (int k = 0; k < b->ncls; k++) { hx_stream_reset(&b->params[k], k, &init[k]); b->cls_fp.push_back(cfg_fingerprint(b->params[k])); }
    if (dev_alloc(b, b->d_init, sizeof(HxStream) * b->ncls) != 0) return -1;
    HIPCHK(hipMemcpy(b->d_init, init.data(), sizeof(HxStream) * b->ncls, hipMemcpyHostToDevice));
    b->slot_mark.assign(b->S, 0);
    return 0;
}
int slots_src_init(hx_batch *b)
{
    std::vector<unsigned long long> fp(b->S), pfp(b->nsrc);
    for (int k = 0; k < b->nsrc; k++) pfp[k] = plan_fingerprint(b->src_plans[k]);
    for (int s = 0; s < b->S; s++) fp[s] = pfp[b->src_cls[s]];
    if (dev_alloc(b, b->d_src_fp, (long long) sizeof(unsigned long long) * b->S) != 0 ||
        dev_alloc(b, b->d_plan_fp, (long long) sizeof(unsigned long long) * b->nsrc) != 0) return -1;
    HIPCHK(hipMemcpy(b->d_src_fp, fp.data(), sizeof(unsigned long long) * b->S, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->d_plan_fp, pfp.data(), sizeof(unsigned long long) * b->nsrc, hipMemcpyHostToDevice));
    return 0;
}

// why slot i does not take the blob at `host` (hx_last_error is set), or 0
static int blob_refused(const hx_batch *b, int i, const void *host, const char *prefix)
{
    const unsigned magic = b->nsrc ? HX_STATE_MAGIC_SRC : HX_STATE_MAGIC;
    const char *why = nullptr;
    HxStateHeader in;
    memcpy(&in, host, sizeof(in));
    unsigned long long fp = 0;
    if (b->nsrc) memcpy(&fp, (const char *) host + HX_STATE_OFF_SRC_FP, sizeof(fp));
    if ((in.magic == HX_STATE_MAGIC) != (magic == HX_STATE_MAGIC) && (in.magic == HX_STATE_MAGIC || in.magic == HX_STATE_MAGIC_SRC))
        why = b->nsrc ? "a stream-state blob of a batch without converter: a converting batch does not take it" : "a stream-state blob of a converting batch: this batch has no converter";
    else if (in.magic != magic || in.version != HX_STATE_VERSION || in.state_bytes != (unsigned) sizeof(HxStream)) why = "not a stream-state blob of this library build";
    else if (in.cfg != b->cls_fp[b->cls_of[i]]) why = "the stream state was saved under a different configuration than slot's";
    else if (fp != (b->nsrc ? plan_fingerprint(b->src_plans[b->src_cls[i]]) : 0)) why = "the stream state was saved with a different converter (source format, rates or layout) than slot's";
    if (!why) return 0;
    set_err("%s", (std::string(prefix) + why).c_str());
    return -1;
}

enum SlotOp { SLOT_RESET, SLOT_GATHER, SLOT_SCATTER };

// The refusals, made before anything is allocated, uploaded or launched; hx_last_error names the entry.
// blobs: the operation moves blobs ([n][stride] at `blobs`; device: in device memory)
static int slots_check(hx_batch *b, const int *idx, int n, bool blobs, const void *p_blobs, long long stride, bool device)
{
    char msg[160];
#define REFUSE(...) do { snprintf(msg, sizeof msg, __VA_ARGS__); set_err("%s", msg); return -1; } while (0)
    if (!b) { set_err("null batch"); return -1; }
    if (check_poisoned(b) != 0) return -1;
    if (n < 0) REFUSE("n = %d: the number of listed slots cannot be negative", n);
    if (n > 0 && !idx) { set_err("idx is null with n > 0"); return -1; }
    if (blobs && device && b->nsrc) {
        set_err("a converting batch has no device-blob calls (the host's converter call counts are authoritative): use hx_batch_get / set_stream_states");
        return -1;
    }
    if (blobs) {
        if (stride < hx_batch_stream_state_bytes(b) || (stride & 15) != 0)
            REFUSE("blob_stride %lld: it must be a multiple of 16 and at least hx_batch_stream_state_bytes = %lld (hx_batch_stream_states_stride)", stride, hx_batch_stream_state_bytes(b));
        if (n > 0 && !p_blobs) { set_err("the blob array is null with n > 0"); return -1; }
        if (device && ((unsigned long long) p_blobs & 15) != 0) { set_err("d_blobs must be 16-byte aligned"); return -1; }
    }
    const long long serial = ++b->slot_serial;
    for (int e = 0; e < n; e++) {
        if (idx[e] < 0 || idx[e] >= b->S) REFUSE("entry %d: slot %d out of range (0 .. %d)", e, idx[e], b->S - 1);
        if (b->slot_mark[idx[e]] == serial) REFUSE("entry %d: slot %d is listed twice", e, idx[e]);
        b->slot_mark[idx[e]] = serial;
    }
#undef REFUSE
    return 0;
}

// One operation on stream q (arguments checked, n > 0).  The entry list goes up through staging copy k of three, in a
// rotation of the slot operations' own; the copy's event is recorded behind the kernel that reads the device list, so
// refilling copy k three operations later waits for that operation as a whole, whatever streams the operations in between
// were made on.
// cfg (a reset): null, or [n] the menu entry each listed slot takes; its entry then carries that menu entry's class and plan
static int slot_op(hx_batch *b, SlotOp op, const int *idx, int n, void *d_blobs, long long stride, hipStream_t q, const int *cfg = nullptr)
{
    HIPCHK(hipSetDevice(b->device));
    Staging &s = b->ent_stage;
    if (!s.d && staging_make(b, s, sizeof(HxSlotEntry) * (size_t) b->S) != 0) return -1;
    Poison poison{b};
    if (b->inflight) {
        if (order_behind_submits(b, q) != 0) return -1;
        b->inflight = false;
    }
    const int k = (int) (b->nslotops++ % 3);
    HxSlotEntry *h = (HxSlotEntry *) staging_take(s, k);
    if (!h) return -1;
    for (int e = 0; e < n; e++) {
        const int cls = cfg ? b->menu_cls[cfg[e]] : b->cls_of[idx[e]];
        h[e] = HxSlotEntry{idx[e], cls, b->cls_fp[cls], b->nsrc ? (cfg ? b->menu_plan[cfg[e]] : b->src_cls[idx[e]]) : 0, 0};
    }
    if (staging_upload(s, k, sizeof(HxSlotEntry) * (size_t) n, q) != 0) return -1;
    SlotArgs a;
    a.ent = s.dev<HxSlotEntry>(k); a.st = b->d_st; a.init = b->d_init; a.sb = b->d_sb; a.sb_row = (2LL * b->maxF + 3) * 576;
    a.src_calls = b->nsrc ? b->d_src_calls : nullptr; a.src_carry = b->d_src_carry; a.src_fp = b->d_src_fp;
    a.src_cls = b->d_src_cls; a.plan_fp = b->d_plan_fp;
    a.S = b->S; a.src_par = b->src_par;
    a.magic = b->nsrc ? HX_STATE_MAGIC_SRC : HX_STATE_MAGIC; a.version = HX_STATE_VERSION;
    a.status = b->d_status;
    a.recon_state = b->d_recon_state;
    a.blob_words = stride / 8;
    // words behind the header that the kernel walks (a reset leaves the converter's carried samples - call 0 of any plan
    // reads none - and its lane behind the two call counts writes the slot's plan and plan fingerprint)
    const long long state_words = b->nsrc ? HX_SLOT_SRC_CARRY_WORD + HX_SLOT_SRC_CARRY_WORDS : HX_SLOT_SRC_WORD;
    const long long words = op == SLOT_GATHER ? a.blob_words : op == SLOT_SCATTER ? state_words : b->nsrc ? HX_SLOT_SRC_CARRY_WORD + 1 : HX_SLOT_SRC_WORD;
    a.chunks = (int) ((words + HX_SLOT_CHUNK - 1) / HX_SLOT_CHUNK);
    const dim3 grid((unsigned) ((long long) n * a.chunks));
    if (op == SLOT_RESET) LAUNCH(k_slot_reset, grid, dim3(256), q, a);
    else if (op == SLOT_GATHER) LAUNCH(k_slot_gather, grid, dim3(256), q, a, (uint2 *) d_blobs);
    else LAUNCH(k_slot_scatter, grid, dim3(256), q, a, (const uint2 *) d_blobs);
    if (staging_done(s, k, q) != 0) return -1;
    return poison.ok();
}

// n slots start new streams on stream q, slot idx[e] of menu entry cfg[e] (cfg null, hx_batch_reset_streams: of the entry it
// runs); wait (hx_batch_reset_stream): behind everything in flight, and done when it returns.  The host's view of the
// slots - entry, class, plan, converter call count - moves here, when the call is made; the device follows in stream order.
int assign_slots(hx_batch *b, const int *idx, const int *cfg, int n, void *stream, bool wait)
{
    const hipStream_t q = (hipStream_t) stream;
    if (slots_check(b, idx, n, false, nullptr, 0, false) != 0) return -1;
    for (int e = 0; cfg && e < n; e++)
        if (cfg[e] < 0 || cfg[e] >= (int) b->menu_cls.size()) {
            char msg[96];
            snprintf(msg, sizeof msg, "entry %d: configuration %d out of range (0 .. %d)", e, cfg[e], (int) b->menu_cls.size() - 1);
            set_err("%s", msg);
            return -1;
        }
    if (n == 0) return 0;
    if (wait && drain(b) != 0) return -1;
    if (slot_op(b, SLOT_RESET, idx, n, nullptr, 0, q, cfg) != 0) return -1;
    for (int e = 0; e < n; e++) {
        const int s = idx[e];
        if (cfg) { b->cfg_of[s] = cfg[e]; b->cls_of[s] = b->menu_cls[cfg[e]]; }
        if (b->nsrc) {          // (the converters start over: the host's count is the authoritative one)
            if (cfg) b->src_cls[s] = b->menu_plan[cfg[e]];
            b->src_calls[s] = 0;
        }
    }
    if (wait) HIPCHK(hipStreamSynchronize(q));
    return 0;
}
extern "C" int hx_batch_reset_streams(hx_batch *b, const int *idx, int n, void *stream) { return assign_slots(b, idx, nullptr, n, stream, false); }
extern "C" int hx_batch_reset_stream(hx_batch *b, int i) { return assign_slots(b, &i, nullptr, 1, nullptr, true); }
extern "C" int hx_batch_assign_streams(hx_batch *b, const int *idx, const int *cfg, int n, void *stream)
{
    if (b && n > 0 && !cfg) { set_err("cfg is null with n > 0"); return -1; }
    return assign_slots(b, idx, cfg, n, stream, false);
}

extern "C" int hx_batch_get_stream_states_device(hx_batch *b, const int *idx, int n, void *d_blobs, long long blob_stride, void *stream)
{
    if (slots_check(b, idx, n, true, d_blobs, blob_stride, true) != 0) return -1;
    return n == 0 ? 0 : slot_op(b, SLOT_GATHER, idx, n, d_blobs, blob_stride, (hipStream_t) stream);
}
extern "C" int hx_batch_set_stream_states_device(hx_batch *b, const int *idx, int n, const void *d_blobs, long long blob_stride, void *stream)
{
    if (slots_check(b, idx, n, true, d_blobs, blob_stride, true) != 0) return -1;
    return n == 0 ? 0 : slot_op(b, SLOT_SCATTER, idx, n, (void *) d_blobs, blob_stride, (hipStream_t) stream);
}

// The host-blob calls: synchronous (they wait for the work in flight first), one launch and one copy whatever n is, through
// device staging [n][stride] that grows with n.  A restore is all or nothing: every header is checked on the host before
// anything is written, so no blob of it can set status bit 32.  What crosses between the staging and the caller's memory is
// the blobs up to the end of the last one's state and not a byte more; the list form of a save writes the zeros from there to
// the stride on the host.  one (the single-slot calls): the caller's buffer ends with the state - no zeros behind it - and
// a refusal names no entry.
static int host_blobs(hx_batch *b, SlotOp op, const int *idx, int n, void *blobs, long long stride, bool one)
{
    if (slots_check(b, idx, n, true, blobs, stride, false) != 0) return -1;
    if (n == 0) return 0;
    for (int e = 0; e < n && op == SLOT_SCATTER; e++) {
        char prefix[32] = "";
        if (!one) snprintf(prefix, sizeof prefix, "entry %d: ", e);
        if (blob_refused(b, idx[e], (const char *) blobs + (long long) e * stride, prefix) != 0) return -1;
    }
    if (drain(b) != 0) return -1;
    const long long need = hx_batch_stream_state_bytes(b), nb = (long long) (n - 1) * stride + need;
    if (dev_grow(b, b->d_blobs, b->blobs_cap, (long long) n * stride) != 0) return -1;
    if (op == SLOT_SCATTER) HIPCHK(hipMemcpy(b->d_blobs, blobs, (size_t) nb, hipMemcpyHostToDevice));
    if (slot_op(b, op, idx, n, b->d_blobs, stride, nullptr) != 0) return -1;
    HIPCHK(hipStreamSynchronize(nullptr));
    if (op == SLOT_GATHER) {
        HIPCHK(hipMemcpy(blobs, b->d_blobs, (size_t) nb, hipMemcpyDeviceToHost));
        if (!one) memset((char *) blobs + nb, 0, (size_t) (stride - need));
    }
    for (int e = 0; e < n && op == SLOT_SCATTER && b->nsrc; e++)        // (the host's converter call count is the authoritative one)
        memcpy(&b->src_calls[idx[e]], (const char *) blobs + (long long) e * stride + HX_STATE_OFF_SRC_CALLS, sizeof(long long));
    return 0;
}
extern "C" int hx_batch_get_stream_states(hx_batch *b, const int *idx, int n, void *blobs, long long blob_stride)
{
    return host_blobs(b, SLOT_GATHER, idx, n, blobs, blob_stride, false);
}
extern "C" int hx_batch_set_stream_states(hx_batch *b, const int *idx, int n, const void *blobs, long long blob_stride)
{
    return host_blobs(b, SLOT_SCATTER, idx, n, (void *) blobs, blob_stride, false);
}
extern "C" int hx_batch_get_stream_state(hx_batch *b, int i, void *dst)
{
    return host_blobs(b, SLOT_GATHER, &i, 1, dst, hx_batch_stream_states_stride(b), true);
}
extern "C" int hx_batch_set_stream_state(hx_batch *b, int i, const void *src)
{
    return host_blobs(b, SLOT_SCATTER, &i, 1, (void *) src, hx_batch_stream_states_stride(b), true);
}

// ---- the file ledger's slot operations (include/hmp3_amd.h; kernels: hx_ledger.hip) ----
// hx_batch_ledger_begin and the two reads list slots like the operations above and share their refusals, their staging
// rotation and their ordering: on the caller's stream behind everything in flight, the deferred packing - and with it the
// previous occupant's last update, which travels with that packing - out first.

// One ledger operation on stream q (arguments checked, n > 0): open == null: a gather into d_out
static int ledger_op(hx_batch *b, const int *idx, const HX_LEDGER_OPEN *open, int n, HX_LEDGER *d_out, hipStream_t q)
{
    HIPCHK(hipSetDevice(b->device));
    Staging &s = b->ent_stage;
    if (!s.d && staging_make(b, s, sizeof(HxSlotEntry) * (size_t) b->S) != 0) return -1;
    if (!b->d_ledger) {         // (the first begin: all records closed, in stream order in front of its kernel)
        HX_LEDGER *led = nullptr;
        if (dev_alloc(b, led, (long long) sizeof(HX_LEDGER) * b->S) != 0) return -1;
        HIPCHK(hipMemsetAsync(led, 0, sizeof(HX_LEDGER) * (size_t) b->S, q));
        b->d_ledger = led;
        b->led_live.assign(b->S, 0);
    }
    Poison poison{b};
    if (b->inflight) {
        if (order_behind_submits(b, q) != 0) return -1;
        b->inflight = false;
    }
    const int k = (int) (b->nslotops++ % 3);
    HxLedgerEntry *h = (HxLedgerEntry *) staging_take(s, k);
    if (!h) return -1;
    for (int e = 0; e < n; e++) h[e] = open ? HxLedgerEntry{idx[e], open[e].ncalls, open[e].head_bytes, open[e].flags, frames_per_block(b->params[b->cls_of[idx[e]]])} : HxLedgerEntry{idx[e], 0, 0, 0, 0};
    if (staging_upload(s, k, sizeof(HxLedgerEntry) * (size_t) n, q) != 0) return -1;
    if (open) {
        LAUNCH(k_ledger_begin, dim3((unsigned) n), dim3(256), q, b->d_ledger, (const HxLedgerEntry *) s.dev<HxLedgerEntry>(k));
        // (file images: the opened slots' length words restart, and say whether the record has an image)
        if (b->files.fw) LAUNCH(k_file_begin, dim3((unsigned) ((n + 255) / 256)), dim3(256), q, (uint2 *) b->files.fw, (const HxLedgerEntry *) s.dev<HxLedgerEntry>(k), n, b->files.img ? 1u : 0u);
    } else LAUNCH(k_ledger_gather, dim3((unsigned) n), dim3(256), q, (const HX_LEDGER *) b->d_ledger, (const HxLedgerEntry *) s.dev<HxLedgerEntry>(k), d_out);
    if (staging_done(s, k, q) != 0) return -1;
    return poison.ok();
}

int ledger_begin(hx_batch *b, const int *idx, const HX_LEDGER_OPEN *open, int n, void *stream, bool wait)
{
    const hipStream_t q = (hipStream_t) stream;
    if (slots_check(b, idx, n, false, nullptr, 0, false) != 0) return -1;
    if (n > 0 && !open) { set_err("open is null with n > 0"); return -1; }
    for (int e = 0; e < n; e++)
        if (open[e].ncalls < 1 || open[e].head_bytes < 0) {
            char msg[96];
            snprintf(msg, sizeof msg, open[e].ncalls < 1 ? "entry %d: ncalls < 1" : "entry %d: head_bytes < 0", e);
            set_err("%s", msg);
            return -1;
        }
    if (n == 0) return 0;
    if (wait && drain(b) != 0) return -1;
    if (ledger_op(b, idx, open, n, nullptr, q) != 0) return -1;
    if (b->led_head.empty()) b->led_head.assign(b->S, 0);
    if (b->led_img.empty()) b->led_img.assign(b->S, 0);
    for (int e = 0; e < n; e++) { b->led_live[idx[e]] = 1; b->led_head[idx[e]] = open[e].head_bytes; b->led_img[idx[e]] = b->files.img ? 1 : 0; }     // (the host's view moves when the call is made, like a slot's configuration)
    if (wait) HIPCHK(hipStreamSynchronize(q));
    return 0;
}
extern "C" int hx_batch_ledger_begin(hx_batch *b, const int *idx, const HX_LEDGER_OPEN *open, int n, void *stream)
{
    return ledger_begin(b, idx, open, n, stream, false);
}

// a batch without a ledger has [S] closed records: all zero
extern "C" int hx_batch_ledger_read_device(hx_batch *b, const int *idx, int n, HX_LEDGER *d_out, void *stream)
{
    if (slots_check(b, idx, n, false, nullptr, 0, false) != 0) return -1;
    if (n > 0 && !d_out) { set_err("d_out is null with n > 0"); return -1; }
    if (((unsigned long long) d_out & 15) != 0) { set_err("d_out must be 16-byte aligned"); return -1; }
    if (n == 0) return 0;
    if (!b->d_ledger) {
        HIPCHK(hipSetDevice(b->device));
        HIPCHK(hipMemsetAsync(d_out, 0, sizeof(HX_LEDGER) * (size_t) n, (hipStream_t) stream));
        return 0;
    }
    return ledger_op(b, idx, nullptr, n, d_out, (hipStream_t) stream);
}

// synchronous: behind everything in flight, one gather launch into device staging, one copy; a record it shows ended is no
// longer live for the host
int ledger_read(hx_batch *b, const int *idx, int n, HX_LEDGER *out)
{
    if (slots_check(b, idx, n, false, nullptr, 0, false) != 0) return -1;
    if (n > 0 && !out) { set_err("out is null with n > 0"); return -1; }
    if (n == 0) return 0;
    if (!b->d_ledger) { memset(out, 0, sizeof(HX_LEDGER) * (size_t) n); return 0; }
    if (drain(b) != 0) return -1;
    if (dev_grow(b, b->d_blobs, b->blobs_cap, (long long) sizeof(HX_LEDGER) * n) != 0) return -1;
    if (ledger_op(b, idx, nullptr, n, (HX_LEDGER *) b->d_blobs, nullptr) != 0) return -1;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(out, b->d_blobs, sizeof(HX_LEDGER) * (size_t) n, hipMemcpyDeviceToHost));
    for (int e = 0; e < n; e++) if (out[e].ended || !out[e].open) b->led_live[idx[e]] = 0;
    return 0;
}
extern "C" int hx_batch_ledger_read(hx_batch *b, const int *idx, int n, HX_LEDGER *out) { return ledger_read(b, idx, n, out); }

// ---- file images (include/hmp3_amd.h, "file images"; kernels: hx_fileimg.hip) ----
// The images are one allocation, [S][pitch]; the length words fw [S][2] are made at the first switch-on and kept.  Switching
// is synchronous and refused while the host counts a record as live, so no call in flight or to come holds a record that
// points into the images that go.  A switch is all or nothing: the new images are allocated while the old ones still stand,
// so a refused allocation changes nothing - at the price that a change of cap needs both sets on the device for a moment (a
// caller short of memory switches off first, with cap = 0).

static void dev_release(hx_batch *b, void *p)
{
    if (!p) return;
    hipFree(p);
    for (void *&m : b->mem) if (m == p) { m = b->mem.back(); b->mem.pop_back(); break; }
}
int images_reserve(hx_batch *b, long long cap, FileImages &next)
{
    next = FileImages();
    if (!b) { set_err("null batch"); return -1; }
    if (check_poisoned(b) != 0) return -1;
    if (cap < 0) { set_err("cap < 0"); return -1; }
    for (int s = 0; s < (int) b->led_live.size(); s++)
        if (b->led_live[s]) {
            char msg[160];
            snprintf(msg, sizeof msg, "stream %d has a live ledger record: file images are switched between files (read or poll the record's end first)", s);
            set_err("%s", msg);
            return -1;
        }
    if (cap == 0) return 0;
    if (cap > LLONG_MAX - 15 || ((cap + 15) & ~15LL) > LLONG_MAX / b->S) { set_err("the file images do not fit the device's memory"); return -1; }
    HIPCHK(hipSetDevice(b->device));
    // (a refused hipMalloc leaves its error with the runtime, where the next launch check of this thread would find it and
    // poison the batch: it is read away here, so that a refusal leaves the batch as usable as it was)
    if (!b->files.fw) {
        if (dev_alloc(b, b->files.fw, (long long) sizeof(unsigned) * 2 * b->S) != 0) { (void) hipGetLastError(); return -1; }
        HIPCHK(hipMemset(b->files.fw, 0, sizeof(unsigned) * 2 * (size_t) b->S));
    }
    next.cap = cap;
    next.pitch = (cap + 15) & ~15LL;
    if (dev_alloc(b, next.img, next.pitch * b->S) != 0) {
        (void) hipGetLastError();
        set_err("the file images do not fit the device's memory");
        next = FileImages();
        return -1;
    }
    return 0;
}
void images_drop(hx_batch *b, FileImages &next)
{
    dev_release(b, next.img);
    next = FileImages();
}
int images_commit(hx_batch *b, const FileImages &next)
{
    if (drain(b) != 0) return -1;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned *fw = b->files.fw;
    if (fw) HIPCHK(hipMemset(fw, 0, sizeof(unsigned) * 2 * (size_t) b->S));
    // (nothing fails from here on: a commit that returns -1 has not taken `next`)
    dev_release(b, b->files.img);
    dev_release(b, b->d_many);          // (the fetch of many's staging goes with the images it was sized for)
    b->d_many = nullptr; b->many_cap = 0;
    std::fill(b->led_img.begin(), b->led_img.end(), 0);     // (records begun before a switch have no image)
    b->files = next;
    b->files.fw = fw;
    return 0;
}
extern "C" int hx_batch_file_images(hx_batch *b, long long cap)
{
    FileImages next;
    if (images_reserve(b, cap, next) != 0) return -1;
    return images_commit(b, next);
}
extern "C" long long hx_batch_file_image_cap(const hx_batch *b) { return b ? b->files.cap : 0; }
extern "C" unsigned char *hx_batch_file_image_ptr(hx_batch *b, int i)
{
    return (b && b->files.img && i >= 0 && i < b->S) ? b->files.img + (long long) i * b->files.pitch : nullptr;
}

// the briefs of all slots on stream q into d_out (ordered like a ledger operation: behind everything in flight)
static int brief_op(hx_batch *b, HX_LEDGER_BRIEF *d_out, hipStream_t q)
{
    HIPCHK(hipSetDevice(b->device));
    Poison poison{b};
    if (b->inflight) {
        if (order_behind_submits(b, q) != 0) return -1;
        b->inflight = false;
    }
    LAUNCH(k_ledger_brief, dim3((unsigned) ((b->S + 255) / 256)), dim3(256), q, (const HX_LEDGER *) b->d_ledger, (const uint2 *) b->files.fw, d_out, b->S);
    return poison.ok();
}
extern "C" int hx_batch_ledger_poll_device(hx_batch *b, HX_LEDGER_BRIEF *d_out, void *stream)
{
    if (!b) { set_err("null batch"); return -1; }
    if (check_poisoned(b) != 0) return -1;
    if (!d_out) { set_err("d_out is null"); return -1; }
    if (((unsigned long long) d_out & 15) != 0) { set_err("d_out must be 16-byte aligned"); return -1; }
    return brief_op(b, d_out, (hipStream_t) stream);
}
// synchronous: behind everything in flight, one launch into device staging, one copy; a record it shows ended is no longer
// live for the host
int ledger_poll(hx_batch *b, HX_LEDGER_BRIEF *out)
{
    if (!b) { set_err("null batch"); return -1; }
    if (check_poisoned(b) != 0) return -1;
    if (!out) { set_err("out is null"); return -1; }
    if (drain(b) != 0) return -1;
    if (dev_grow(b, b->d_blobs, b->blobs_cap, (long long) sizeof(HX_LEDGER_BRIEF) * b->S) != 0) return -1;
    if (brief_op(b, (HX_LEDGER_BRIEF *) b->d_blobs, nullptr) != 0) return -1;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(out, b->d_blobs, sizeof(HX_LEDGER_BRIEF) * (size_t) b->S, hipMemcpyDeviceToHost));
    for (int s = 0; s < (int) b->led_live.size(); s++) if (out[s].ended || !out[s].open) b->led_live[s] = 0;
    return 0;
}
extern "C" int hx_batch_ledger_poll(hx_batch *b, HX_LEDGER_BRIEF *out) { return ledger_poll(b, out); }

extern "C" long long hx_batch_file_fetch(hx_batch *b, int i, unsigned char *dst, long long dst_cap)
{
    if (!b) { set_err("null batch"); return -1; }
    if (check_poisoned(b) != 0) return -1;
    if (!b->files.img) { set_err("file images are off (hx_batch_file_images)"); return -1; }
    if (i < 0 || i >= b->S) { set_err("stream index out of range"); return -1; }
    if (!dst) { set_err("dst is null"); return -1; }
    if (drain(b) != 0) return -1;
    HIPCHK(hipSetDevice(b->device));
    unsigned w[2] = {0, 0};
    HIPCHK(hipMemcpy(w, b->files.fw + 2 * (size_t) i, sizeof w, hipMemcpyDeviceToHost));
    const long long head = b->led_head.empty() ? 0 : b->led_head[i], total = head + (long long) w[0];
    if (total > dst_cap) {
        char msg[128];
        snprintf(msg, sizeof msg, "stream %d: the file's %lld bytes do not fit dst_cap %lld", i, total, dst_cap);
        set_err("%s", msg);
        return -1;
    }
    if (w[0]) HIPCHK(hipMemcpy(dst + head, b->files.img + (long long) i * b->files.pitch + head, (size_t) w[0], hipMemcpyDeviceToHost));
    return total;
}

// ---- finished files (include/hmp3_amd.h, "finished files"; kernels: hx_fileimg.hip) ----
// hx_batch_file_tags is a slot operation like hx_batch_ledger_begin; its entries are larger than a slot entry and go through
// a staging of their own, in the same rotation.  The fetch of many lists slots like a ledger read.

static int not_capturing(hipStream_t q, const char *what)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(q, &cs) != hipSuccess) { (void) hipGetLastError(); return 0; }    // (the null stream while another captures: the call's own launches will say)
    if (cs == hipStreamCaptureStatusNone) return 0;
    set_err("%s is not made under stream capture", what);
    return -1;
}

int files_refused(const hx_batch *b, const int *idx, const HX_FILE_TAG *tags, int n, const int *entry, int first)
{
    char msg[192];
    if (!b->files.img) { set_err("file images are off (hx_batch_file_images)"); return -1; }
    for (int e = 0; e < n && tags; e++) {
        const int s = idx[e], en = entry ? entry[e] : e, name = first + s;
        if (b->led_img.empty() || !b->led_img[s]) {
            snprintf(msg, sizeof msg, "entry %d: slot %d's record was not begun with an image (hx_batch_ledger_begin while images are on)", en, name);
            set_err("%s", msg);
            return -1;
        }
        const int size = hx_file_tag_bytes(&tags[e]);
        if (size != b->led_head[s]) {
            snprintf(msg, sizeof msg, "entry %d: the tag frame takes %d bytes, slot %d's record was begun with head_bytes %d", en, size, name, b->led_head[s]);
            set_err("%s", msg);
            return -1;
        }
    }
    return 0;
}

int file_tags(hx_batch *b, const int *idx, const HX_FILE_TAG *tags, int n, void *stream, bool wait)
{
    const hipStream_t q = (hipStream_t) stream;
    if (slots_check(b, idx, n, false, nullptr, 0, false) != 0) return -1;
    if (n > 0 && !tags) { set_err("tags is null with n > 0"); return -1; }
    if (n == 0) return 0;
    if (files_refused(b, idx, tags, n, nullptr, 0) != 0) return -1;
    HIPCHK(hipSetDevice(b->device));
    if (not_capturing(q, "hx_batch_file_tags") != 0) return -1;
    int live = 0;
    for (int e = 0; e < n; e++) live += b->led_head[idx[e]] > 0;
    if (!live) return 0;        // (no listed slot has a head room: nothing to write)
    if (wait && drain(b) != 0) return -1;
    Staging &s = b->tag_stage;
    if (!s.d && staging_make(b, s, sizeof(HxFileTagEntry) * (size_t) b->S) != 0) return -1;
    Poison poison{b};
    if (b->inflight) {
        if (order_behind_submits(b, q) != 0) return -1;
        b->inflight = false;
    }
    const int k = (int) (b->nslotops++ % 3);
    HxFileTagEntry *h = (HxFileTagEntry *) staging_take(s, k);
    if (!h) return -1;
    int m = 0;
    for (int e = 0; e < n; e++) {
        if (b->led_head[idx[e]] <= 0) continue;
        h[m] = HxFileTagEntry{idx[e], {0, 0, 0}, {0, 0, 0, 0, 0, 0}};
        memcpy(h[m].tag, &tags[e], sizeof(HX_FILE_TAG));
        m++;
    }
    if (staging_upload(s, k, sizeof(HxFileTagEntry) * (size_t) m, q) != 0) return -1;
    LAUNCH(k_file_tag, dim3((unsigned) m), dim3(256), q, (const HX_LEDGER *) b->d_ledger, (const uint2 *) b->files.fw, b->files.img, b->files.pitch, b->files.cap,
           (const HxFileTagEntry *) s.dev<HxFileTagEntry>(k));
    if (staging_done(s, k, q) != 0) return -1;
    if (poison.ok() != 0) return -1;
    if (wait) HIPCHK(hipStreamSynchronize(q));
    return 0;
}
extern "C" int hx_batch_file_tags(hx_batch *b, const int *idx, const HX_FILE_TAG *tags, int n, void *stream)
{
    return file_tags(b, idx, tags, n, stream, false);
}

// the list on stream q through the slot operations' staging (copy k of the rotation, returned), then k_file_off into d_off
static int files_off_op(hx_batch *b, const int *idx, int n, long long *d_off, long long dst_cap, hipStream_t q, int &k)
{
    Staging &s = b->ent_stage;
    if (!s.d && staging_make(b, s, sizeof(HxSlotEntry) * (size_t) b->S) != 0) return -1;
    if (b->inflight) {
        if (order_behind_submits(b, q) != 0) return -1;
        b->inflight = false;
    }
    k = (int) (b->nslotops++ % 3);
    HxLedgerEntry *h = (HxLedgerEntry *) staging_take(s, k);
    if (!h) return -1;
    for (int e = 0; e < n; e++) h[e] = HxLedgerEntry{idx[e], 0, 0, 0, 0};
    if (staging_upload(s, k, sizeof(HxLedgerEntry) * (size_t) n, q) != 0) return -1;
    LAUNCH(k_file_off, dim3(1), dim3(1024), q, (const HxLedgerEntry *) s.dev<HxLedgerEntry>(k), n, (const HX_LEDGER *) b->d_ledger, (const uint2 *) b->files.fw,
           b->files.cap, d_off, dst_cap, b->d_status);
    return 0;
}
// ... and k_file_gather over that list into d_dst; the copy's event goes behind it
static int files_gather_op(hx_batch *b, int n, int k, const long long *d_off, unsigned char *d_dst, long long dst_cap, hipStream_t q)
{
    Staging &s = b->ent_stage;
    const int chunks = (int) ((b->files.pitch + HX_FILE_GATHER_CHUNK - 1) / HX_FILE_GATHER_CHUNK);
    LAUNCH(k_file_gather, dim3((unsigned) ((long long) n * chunks)), dim3(256), q, (const HxLedgerEntry *) s.dev<HxLedgerEntry>(k), (const HX_LEDGER *) b->d_ledger,
           (const uint2 *) b->files.fw, (const unsigned char *) b->files.img, b->files.pitch, b->files.cap, d_off, d_dst, dst_cap, chunks);
    return staging_done(s, k, q);
}

extern "C" int hx_batch_file_gather_device(hx_batch *b, const int *idx, int n, unsigned char *d_dst, long long dst_cap, long long *d_off, void *stream)
{
    const hipStream_t q = (hipStream_t) stream;
    if (slots_check(b, idx, n, false, nullptr, 0, false) != 0) return -1;
    if (n > 0 && (!d_dst || !d_off)) { set_err("d_dst or d_off is null with n > 0"); return -1; }
    if (((unsigned long long) d_dst & 15) != 0) { set_err("d_dst must be 16-byte aligned"); return -1; }
    if (((unsigned long long) d_off & 7) != 0) { set_err("d_off must be 8-byte aligned"); return -1; }
    if (dst_cap < 0) { set_err("dst_cap < 0"); return -1; }
    if (n == 0) return 0;
    if (files_refused(b, idx, nullptr, n, nullptr, 0) != 0) return -1;
    HIPCHK(hipSetDevice(b->device));
    if (not_capturing(q, "hx_batch_file_gather_device") != 0) return -1;
    Poison poison{b};
    int k = 0;
    if (files_off_op(b, idx, n, d_off, dst_cap, q, k) != 0 || files_gather_op(b, n, k, d_off, d_dst, dst_cap, q) != 0) return -1;
    return poison.ok();
}

int files_many_scan(hx_batch *b, const int *idx, int n, long long *off)
{
    if (drain(b) != 0) return -1;
    HIPCHK(hipSetDevice(b->device));
    if (!b->d_many_off && dev_alloc(b, b->d_many_off, (long long) sizeof(long long) * (b->S + 1)) != 0) return -1;
    Poison poison{b};
    if (files_off_op(b, idx, n, b->d_many_off, LLONG_MAX, nullptr, b->many_k) != 0) return -1;
    if (staging_done(b->ent_stage, b->many_k, nullptr) != 0) return -1;       // (a refused fetch launches no gather behind it)
    HIPCHK(hipMemcpy(off, b->d_many_off, sizeof(long long) * (size_t) (n + 1), hipMemcpyDeviceToHost));
    return poison.ok();
}
int files_many_bring(hx_batch *b, int n, long long total, unsigned char *dst)
{
    if (total <= 0) return 0;
    HIPCHK(hipSetDevice(b->device));
    if (dev_grow(b, b->d_many, b->many_cap, total) != 0) { (void) hipGetLastError(); return -1; }
    Poison poison{b};
    if (files_gather_op(b, n, b->many_k, b->d_many_off, b->d_many, total, nullptr) != 0) return -1;
    HIPCHK(hipMemcpy(dst, b->d_many, (size_t) total, hipMemcpyDeviceToHost));
    return poison.ok();
}
extern "C" long long hx_batch_file_fetch_many(hx_batch *b, const int *idx, int n, unsigned char *dst, long long dst_cap, long long *off)
{
    if (slots_check(b, idx, n, false, nullptr, 0, false) != 0) return -1;
    if (n > 0 && (!dst || !off)) { set_err("dst or off is null with n > 0"); return -1; }
    if (n == 0) { if (off) off[0] = 0; return 0; }
    if (files_refused(b, idx, nullptr, n, nullptr, 0) != 0) return -1;
    if (files_many_scan(b, idx, n, off) != 0) return -1;
    if (off[n] > dst_cap) {
        char msg[128];
        snprintf(msg, sizeof msg, "the files' %lld bytes do not fit dst_cap %lld", off[n], dst_cap);
        set_err("%s", msg);
        return -1;
    }
    if (files_many_bring(b, n, off[n], dst) != 0) return -1;
    return off[n];
}
