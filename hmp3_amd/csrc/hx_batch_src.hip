// hx_batch_src.hip - converting batches: every stream's source goes through its converter on the GPU (k_src, hx_src.hip)
// into fp32 PCM at the encode rate, which the fp32 path encodes.  The host keeps each stream's converter call count: every
// phase of the converter is a closed form of it (hx_src.h), so the host knows each call's input extent without converting
// anything.
#include <string>
#include "hx_rt.h"

int src_menu(const HX_E_CONTROL *ec, const HX_SOURCE *src, int nmenu, const MenuNames &names, std::vector<HX_E_CONTROL> &ecs,
             std::vector<HxSrcPlan> &plans, std::vector<int> &menu_plan)
{
    ecs.resize(nmenu);
    menu_plan.resize(nmenu);
    hx_src *conv = hx_src_create();
    for (int j = 0; j < nmenu; j++) {
        const HX_SOURCE &sc = src[j];
        HxSrcPlan p;
        if (!src_encode_control(ec + j, sc.bits, sc.is_float, sc.mpeg_select, sc.mono_convert, conv, &ecs[j]) || !hx_src_plan(conv, &p)) {
            char msg[64] = "";
            if (names.src_label) snprintf(msg, sizeof msg, "%s %d: ", names.src_label, names.origin ? names.origin[j] : j);
            const std::string why = hx_last_error();
            set_err("%s", (msg + why).c_str());
            hx_src_destroy(conv);
            return -1;
        }
        int k = -1;
        for (size_t i = 0; i < plans.size(); i++) if (memcmp(&plans[i], &p, sizeof(p)) == 0) { k = (int) i; break; }
        if (k < 0) { plans.push_back(p); k = (int) plans.size() - 1; }
        menu_plan[j] = k;
    }
    hx_src_destroy(conv);
    return 0;
}

// the converter of a batch whose encoder part stands: LDS layout, buffers and tables over all of the menu's plans
int src_setup(hx_batch *b, const std::vector<HxSrcPlan> &plans)
{
    const int nstreams = b->S, max_frames = b->maxF;
    b->nsrc = (int) plans.size();
    b->src_plans = plans;
    b->src_cls.resize(nstreams);
    for (int s = 0; s < nstreams; s++) b->src_cls[s] = b->menu_plan[b->cfg_of[s]];
    b->src_calls.assign(nstreams, 0);
    // LDS of a workgroup: the input window (source channels, interleaved), the intermediate samples (output channels,
    // case 4) and the filter bank (cases 2 - 4), each sized for the batch's largest plan (batch_create has held every
    // entry's plan against its own encode control's channel count)
    int xf = 0, zf = 0, cf = 0;
    for (const HxSrcPlan &p : plans) {
        if (p.xwin > b->src_xwin) b->src_xwin = p.xwin;
        if (p.zwin > b->src_zwin) b->src_zwin = p.zwin;
        xf = std::max(xf, p.channels * p.xwin);
        zf = std::max(zf, p.nch * p.zwin);
        if (p.ncase >= 2) cf = std::max(cf, p.totcoef);
    }
    b->src_zoff = xf;
    b->src_coff = xf + zf;
    b->src_lds = sizeof(float) * ((size_t) xf + zf + cf);
    if (b->src_lds > 160 * 1024) { set_err("the converter's window does not fit a workgroup's LDS"); return -1; }
    if (b->src_lds > 64 * 1024 && hipFuncSetAttribute((const void *) k_src, hipFuncAttributeMaxDynamicSharedMemorySize, (int) b->src_lds) != hipSuccess) {
        set_err("the converter's window does not fit a workgroup's LDS"); return -1;
    }
    const long long S = nstreams;
    if (dev_alloc(b, b->d_src_plan, sizeof(HxSrcPlan) * plans.size()) || dev_alloc(b, b->d_src_cls, sizeof(int) * S) ||
        dev_alloc(b, b->d_src_calls, sizeof(long long) * 2 * S) || dev_alloc(b, b->d_src_carry, sizeof(float) * 2 * S * 2 * HX_SRC_CARRY) ||
        dev_alloc(b, b->d_src_pcm, sizeof(float) * S * max_frames * 1152 * b->nchan) || dev_alloc(b, b->d_src_off, sizeof(long long) * S * max_frames) ||
        host_alloc(b, b->h_src_off, sizeof(long long) * S * max_frames) != 0)
        return -1;
    if (new_event(b, b->ev_src_off) != 0 || slots_src_init(b) != 0 ||
        hipMemcpy(b->d_src_plan, plans.data(), sizeof(HxSrcPlan) * plans.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b->d_src_cls, b->src_cls.data(), sizeof(int) * S, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(b->d_src_calls, 0, sizeof(long long) * 2 * S) != hipSuccess ||
        hipMemset(b->d_src_carry, 0, sizeof(float) * 2 * S * 2 * HX_SRC_CARRY) != hipSuccess ||
        hipEventRecord(b->ev_src_off, nullptr) != hipSuccess) {
        set_err("HIP error while setting up the converter");
        return -1;
    }
    return 0;
}

// the menu of a batch created from per-stream controls and sources: the distinct pairs, in order of first appearance (a
// refusal names the first stream of the pair, which is the first stream it would have been refused for)
extern "C" hx_batch *hx_batch_create_src(int device, int nstreams, const HX_E_CONTROL *ec, int shared_control, const HX_SOURCE *src,
                                         int shared_source, int max_frames)
{
    if (nstreams <= 0 || max_frames <= 0 || !ec || !src) { set_err("bad arguments"); return nullptr; }
    std::vector<HX_E_CONTROL> mec;
    std::vector<HX_SOURCE> msrc;
    std::vector<int> cfg(nstreams), origin;
    for (int s = 0; s < nstreams; s++) {
        const HX_E_CONTROL &c = shared_control ? ec[0] : ec[s];
        const HX_SOURCE &sc = shared_source ? src[0] : src[s];
        int k = -1;
        for (size_t i = 0; i < mec.size(); i++) if (memcmp(&mec[i], &c, sizeof(c)) == 0 && memcmp(&msrc[i], &sc, sizeof(sc)) == 0) { k = (int) i; break; }
        if (k < 0) { mec.push_back(c); msrc.push_back(sc); origin.push_back(s); k = (int) mec.size() - 1; }
        cfg[s] = k;
    }
    return batch_create(device, nstreams, mec.data(), (int) mec.size(), msrc.data(), cfg.data(), max_frames, MenuNames{"stream", nullptr, origin.data()});
}

extern "C" long long hx_batch_src_schedule(const hx_batch *b, int i, int nframes, long long *in_bytes)
{
    if (!b || !b->nsrc || i < 0 || i >= b->S || nframes < 0) { set_err("bad arguments (or not a converting batch)"); return -1; }
    return hx_src_plan_schedule(&b->src_plans[b->src_cls[i]], b->src_calls[i], nframes, in_bytes);
}

extern "C" long long hx_batch_src_in_stride(const hx_batch *b, int nframes)
{
    if (!b || !b->nsrc || nframes < 0) return 0;
    long long n = 0;
    for (const HxSrcPlan &p : b->src_plans) {
        const long long v = ((long long) nframes * p.cmax + p.xwin) * p.channels * (p.bits / 8);
        if (v > n) n = v;
    }
    return (n + 255) & ~255LL;
}

// argument checks of the converting calls
static int src_check(const hx_batch *b, const void *in, long long in_stride, int nframes, const void *out, long long out_stride, const void *out_bytes, bool outputs)
{
    if (b && !b->nsrc) { set_err("not a converting batch (hx_batch_create_src)"); return -1; }
    if (check_args(b, in, nframes, out, out_stride, out_bytes, outputs) != 0) return -1;
    if (in_stride <= 0) { set_err("in_stride must be positive"); return -1; }
    return 0;
}

// Every call's input extent from the schedule, checked against the row before anything runs.  Consecutive calls: the
// consumption telescopes, and the last call reaches furthest (a call reads at most ntaps - k past its successor's
// start, and the last one reads at least ntaps), so one closed form per stream; with offsets every call is checked.
// Under counts (nfr, host) stream s makes n = nfr[s] calls: its last call is c0 + n - 1, only the offsets f < n are read,
// and a stream with n = 0 reads nothing, offsets included.
int src_extents(const hx_batch *b, long long in_stride, const long long *frame_off, int nframes, const int *nfr, int first, long long *used_end)
{
    for (int s = 0; s < b->S; s++) {
        const int n = nfr ? nfr[s] : nframes;
        if (used_end) used_end[s] = 0;
        if (n == 0) continue;
        const HxSrcPlan &p = b->src_plans[b->src_cls[s]];
        const long long fb = (long long) p.channels * (p.bits / 8), c0 = b->src_calls[s];
        long long used, rd;
        int bad = -1;
        long long off = 0;
        if (!frame_off) {
            off = hx_src_consumed(&p, c0, c0 + n - 1) * fb;
            hx_src_call_extent(&p, c0 + n - 1, &used, &rd);
            if (off + rd * fb > in_stride) bad = n - 1;
        } else {
            for (int f = 0; f < n && bad < 0; f++) {
                off = frame_off[(long long) s * nframes + f];
                hx_src_call_extent(&p, c0 + f, &used, &rd);
                if (off < 0 || off + rd * fb > in_stride) bad = f;
            }
        }
        if (bad >= 0) {
            char msg[160];
            snprintf(msg, sizeof msg, "stream %d, call %d: its input [%lld, %lld) does not fit in_stride %lld", first + s, bad, off, off + rd * fb, in_stride);
            set_err("%s", msg);
            return -1;
        }
        if (used_end) used_end[s] = off + used * fb;
    }
    return 0;
}

// The counts of a converting call under counts are the batch's for as long as the call runs: its pass and the copy back of
// a host call (rows_to_host) take them from there, as a plain batch's calls do.  Between calls a converting batch has none.
struct CallCounts {
    hx_batch *b;
    CallCounts(hx_batch *b_, const int *nfr) : b(b_) { if (nfr) b->nfr.assign(nfr, nfr + b->S); }
    ~CallCounts() { b->nfr.clear(); }
};

// one converting call on device buffers (arguments and extents checked by the caller, counts in b->nfr): k_src into
// d_src_pcm, then the fp32 pass over it.  Both read the same device copy of the counts, uploaded in front of k_src.
static int src_encode(hx_batch *b, const unsigned char *d_in, long long in_stride, const long long *frame_off, int nframes,
                      Call c, const long long *used_end, long long *in_used, void *stream)
{
    const int S = b->S;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t q = (hipStream_t) stream;
    Poison poison{b};                   // (from the first upload on)
    if (!b->nfr.empty() && counts_upload_plain(b, q, c.nfr) != 0) return -1;
    if (frame_off) {
        // (entries beyond a stream's count travel as they are: no workgroup reads them)
        const size_t nb = sizeof(long long) * (size_t) S * nframes;
        HIPCHK(hipEventSynchronize(b->ev_src_off));        // (the page-locked copy of the previous call's offsets is on the device)
        memcpy(b->h_src_off, frame_off, nb);
        HIPCHK(hipMemcpyAsync(b->d_src_off, b->h_src_off, nb, hipMemcpyHostToDevice, q));
        HIPCHK(hipEventRecord(b->ev_src_off, q));
    }
    SrcArgs a;
    a.in = d_in; a.in_stride = in_stride; a.off = frame_off ? b->d_src_off : nullptr;
    a.plan = b->d_src_plan; a.cls = b->d_src_cls;
    a.calls_in = b->d_src_calls + (long long) b->src_par * S; a.calls_out = b->d_src_calls + (long long) (1 - b->src_par) * S;
    a.carry_in = b->d_src_carry + (long long) b->src_par * S * 2 * HX_SRC_CARRY;
    a.carry_out = b->d_src_carry + (long long) (1 - b->src_par) * S * 2 * HX_SRC_CARRY;
    a.out = b->d_src_pcm; a.nfr = c.nfr; a.nframes = nframes; a.nch = b->nchan; a.xwin = b->src_xwin; a.zwin = b->src_zwin;
    a.zoff = b->src_zoff; a.coff = b->src_coff; a.status = b->d_status;
    LAUNCH_LDS(k_src, dim3((unsigned) ((long long) S * nframes)), dim3(256), b->src_lds, q, a);
    b->src_par ^= 1;
    for (int s = 0; s < S; s++) b->src_calls[s] += b->nfr.empty() ? nframes : b->nfr[s];
    b->src_lastF = nframes;
    if (in_used) memcpy(in_used, used_end, sizeof(long long) * S);
    if (encode_pass(b, {b->d_src_pcm, true}, nframes, c, stream, PASS_PLAIN) != 0) return -1;
    return poison.ok();
}

// what a converting call checks before anything is allocated, copied, launched or counted: the arguments, the counts'
// range, the optional outputs it would take and every stream's input extent (used_end: see src_extents).  files (the _files
// call): it has no output buffers of the caller's, and its counters and CRCs are the staging's own - nothing of either to check
static int src_checked(hx_batch *b, const void *in, long long in_stride, const long long *frame_off, int nframes, const int *nfr,
                       const void *out, long long out_stride, const void *out_bytes, const OptOut &o, std::vector<long long> &used_end, bool files = false)
{
    if (src_check(b, in, in_stride, nframes, out, out_stride, out_bytes, !files) != 0 || check_counts_arg(nfr, b->S, nframes, 0) != 0 ||
        (!files && check_opt(b, o, nfr) != 0)) return -1;
    used_end.resize(b->S);
    if (src_extents(b, in_stride, frame_off, nframes, nfr, 0, used_end.data()) != 0) return -1;
    return nfr ? counts_buffers(b) : 0;
}

extern "C" int hx_batch_encode_src_counts_device(hx_batch *b, const unsigned char *d_in, long long in_stride, const long long *frame_off,
                                                 int nframes, const int *nfr, unsigned char *d_out, long long out_stride, int *d_out_bytes,
                                                 long long *in_used, void *stream)
{
    std::vector<long long> used_end;
    if (src_checked(b, d_in, in_stride, frame_off, nframes, nfr, d_out, out_stride, d_out_bytes, b ? b->opt : OptOut(), used_end) != 0) return -1;
    CallCounts counts(b, nfr);
    return src_encode(b, d_in, in_stride, frame_off, nframes, call_on(b, d_out, out_stride, d_out_bytes), used_end.data(), in_used, stream);
}
extern "C" int hx_batch_encode_src_device(hx_batch *b, const unsigned char *d_in, long long in_stride, const long long *frame_off,
                                          int nframes, unsigned char *d_out, long long out_stride, int *d_out_bytes,
                                          long long *in_used, void *stream)
{
    return hx_batch_encode_src_counts_device(b, d_in, in_stride, frame_off, nframes, nullptr, d_out, out_stride, d_out_bytes, in_used, stream);
}

// (host_call with a drain before the upload: the staging may still be read by an earlier call)
extern "C" int hx_batch_encode_src_counts_host(hx_batch *b, const unsigned char *in, long long in_stride, const long long *frame_off,
                                               int nframes, const int *nfr, unsigned char *out, long long out_stride, int *out_bytes,
                                               long long *in_used, int *stats, unsigned short *crc)
{
    std::vector<long long> used_end;
    OptOut o = b ? b->opt : OptOut();
    if (stats) o.frame_stats = stats;
    if (crc) { o.crc = crc; if (!stats) o.frame_stats = nullptr; }      // (the host call's CRC comes from the host call's counters)
    if (src_checked(b, in, in_stride, frame_off, nframes, nfr, out, out_stride, out_bytes, o, used_end) != 0) return -1;
    CallCounts counts(b, nfr);
    return host_call(b, in, (long long) b->S * in_stride, true, nframes, out, out_stride, out_bytes, stats, [&](const Call &c) {
        return src_encode(b, (const unsigned char *) b->d_in, in_stride, frame_off, nframes, c, used_end.data(), in_used, nullptr);
    }, nullptr, crc);
}
// The converting host call that brings nothing down but the status (file images): counters and CRCs are the staging's own,
// so the optional outputs it takes always satisfy the ledger.
extern "C" int hx_batch_encode_src_files_host(hx_batch *b, const unsigned char *in, long long in_stride, const long long *frame_off,
                                              int nframes, const int *nfr, long long *in_used)
{
    std::vector<long long> used_end;
    if (check_files(b) != 0) return -1;
    const long long out_stride = hx_batch_out_stride(b, nframes);
    if (src_checked(b, in, in_stride, frame_off, nframes, nfr, nullptr, out_stride, nullptr, b->opt, used_end, true) != 0) return -1;
    CallCounts counts(b, nfr);
    return host_call(b, in, (long long) b->S * in_stride, true, nframes, nullptr, out_stride, nullptr, nullptr, [&](const Call &c) {
        return src_encode(b, (const unsigned char *) b->d_in, in_stride, frame_off, nframes, c, used_end.data(), in_used, nullptr);
    }, nullptr, nullptr, true);
}
extern "C" int hx_batch_encode_src_host(hx_batch *b, const unsigned char *in, long long in_stride, const long long *frame_off,
                                        int nframes, unsigned char *out, long long out_stride, int *out_bytes,
                                        long long *in_used, int *stats)
{
    return hx_batch_encode_src_counts_host(b, in, in_stride, frame_off, nframes, nullptr, out, out_stride, out_bytes, in_used, stats, nullptr);
}
