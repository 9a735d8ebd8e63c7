// hx_batch.hip - the batch of the C ABI (include/hmp3_amd.h) and its launch sequence.
// Owns the device buffers of a batch (subband carry, spectra, psy data, stream state), groups streams into
// configuration classes and launches K1..K8: create / destroy, the pass, submits, host-buffer calls, reads.
#include <cmath>
#include <string>
#include "hx_rt.h"

static thread_local std::string g_err;
void set_err(const char *fmt, const char *a)
{
    char buf[512];
    snprintf(buf, sizeof(buf), fmt, a);
    g_err = buf;
}
extern "C" const char *hx_last_error(void) { return g_err.c_str(); }

// hash of the sources this library was built from (hmp3_amd/build.sh passes it): profiles/ and bench.py use it to tell
// whether committed counter profiles belong to the loaded build
#ifndef HX_BUILD_ID
#define HX_BUILD_ID "unknown"
#endif
extern "C" const char *hx_build_id(void) { return HX_BUILD_ID; }

extern "C" int hx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int flush_pack(hx_batch *b, long long gate_base);

int new_stream(hx_batch *b, hipStream_t &q, int priority)
{
    HIPCHK(priority == INT_MAX ? hipStreamCreateWithFlags(&q, hipStreamNonBlocking) : hipStreamCreateWithPriority(&q, hipStreamNonBlocking, priority));
    b->streams.push_back(q);
    return 0;
}
int new_event(hx_batch *b, hipEvent_t &e)
{
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    b->events.push_back(e);
    return 0;
}

// Buffer set k: front[k], walk[k] and sgn[k] (k = 1: also sgn[2], the third set of signs).
static int alloc_set(hx_batch *b, int k)
{
    const long long S = b->S, NG = 2LL * b->maxF;
    FrontSet &f = b->front[k];
    WalkSet &w = b->walk[k];
    if (dev_alloc(b, f.xr, sizeof(float) * S * NG * 1152) || dev_alloc(b, f.etab, sizeof(float) * S * NG * 128) ||
        dev_alloc(b, f.thr, sizeof(float) * S * NG * 128) || dev_alloc(b, f.x34, sizeof(float) * S * NG * 1152) ||
        dev_alloc(b, f.thrprev, sizeof(float) * S * 128) || dev_alloc(b, f.msbase, sizeof(int) * S * NG) ||
        dev_alloc(b, f.msdec, sizeof(int) * S * NG) || dev_alloc(b, f.bt, S * NG) || dev_alloc(b, f.btprev, S) ||
        dev_alloc(b, f.msflag, S * NG) || dev_alloc(b, f.band, sizeof(HxBandPrep) * S * NG) ||
        dev_alloc(b, w.ixq, sizeof(short) * S * NG * 1152) || dev_alloc(b, w.seg, sizeof(HxSegOut) * S * NG * 2) ||
        dev_alloc(b, w.frm, sizeof(HxFrameOut) * S * NG) || dev_alloc(b, w.slots, sizeof(HxSlot) * S * (NG + HX_SLOTS_EXTRA)))
        return -1;
    w.pre_len = b->d_lens + 2 * k * S;
    w.carry_len = w.pre_len + S;
    if (b->d_recon_state && dev_alloc(b, w.rec, sizeof(HxFrameDebug) * S * b->maxF)) return -1;     // (a set made after the first switch-on of the decoded PCM)
    const long long sgn_bytes = sizeof(unsigned) * S * NG * 2 * HX_SGN_WORDS;
    return (dev_alloc(b, b->sgn[k], sgn_bytes) || (k == 1 && dev_alloc(b, b->sgn[2], sgn_bytes))) ? -1 : 0;
}

// (a packing that cannot be enqueued leaves the batch unusable: Poison)
int drain(hx_batch *b)
{
    HIPCHK(hipSetDevice(b->device));
    if (flush_pack(b, -1) != 0) { b->poisoned = true; return -1; }
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

extern "C" void hx_batch_destroy(hx_batch *b)
{
    if (!b) return;
    hipSetDevice(b->device);
    // A packing that was never asked for (no hx_batch_wait / plain call / status read after the last device-buffer submit)
    // is dropped, not enqueued: it would write into output buffers the caller may have freed already.
    b->pack_job.pending = false;
    hipDeviceSynchronize();
    for (void *p : b->mem) hipFree(p);
    for (hipStream_t q : b->streams) hipStreamDestroy(q);
    for (hipEvent_t e : b->events) hipEventDestroy(e);
    for (auto &pr : b->pending) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    for (void *p : b->pinned) hipHostFree(p);
    delete b;
}

// "<label> <number>: " in front of a refusal that names a menu entry (MenuNames)
static std::string entry_prefix(const char *label, const int *origin, int j)
{
    char msg[64] = "";
    if (label) snprintf(msg, sizeof msg, "%s %d: ", label, origin ? origin[j] : j);
    return msg;
}

hx_batch *batch_create(int device, int nstreams, const HX_E_CONTROL *ec, int nmenu, const HX_SOURCE *src, const int *cfg, int max_frames,
                       const MenuNames &names)
{
    if (nstreams <= 0 || max_frames <= 0 || !ec || nmenu <= 0) { set_err("bad arguments"); return nullptr; }
    for (int s = 0; cfg && s < nstreams; s++)
        if (cfg[s] < 0 || cfg[s] >= nmenu) {
            char msg[96];
            snprintf(msg, sizeof msg, "stream %d: configuration %d out of range (0 .. %d)", s, cfg[s], nmenu - 1);
            set_err("%s", msg);
            return nullptr;
        }
    // a converting batch: every entry's encode control and converter plan
    std::vector<HX_E_CONTROL> ecs;
    std::vector<HxSrcPlan> plans;
    std::vector<int> menu_plan;
    if (src) {
        if (src_menu(ec, src, nmenu, names, ecs, plans, menu_plan) != 0) return nullptr;
        ec = ecs.data();
    }
    hx_batch *b = new hx_batch;
    b->device = device; b->S = nstreams; b->maxF = max_frames;
    b->cls_of.resize(nstreams);
    b->cfg_of.resize(nstreams);
    b->menu_cls.resize(nmenu);
    b->menu_plan = menu_plan;
    // group the menu's entries into configuration classes: everything the batch sizes or decides from its classes is taken
    // over the whole menu, whichever entries the slots start with
    std::vector<HxControl> seen;
    for (int j = 0; j < nmenu; j++) {
        const HxControl *c = (const HxControl *) (ec + j);
        int k = -1;
        for (size_t i = 0; i < seen.size(); i++) if (memcmp(&seen[i], c, sizeof(HxControl)) == 0) { k = (int) i; break; }
        if (k < 0) {
            const std::string pre = entry_prefix(names.cls_label, names.origin, j);
#define REFUSE_ENTRY(text) do { set_err("%s", (pre + (text)).c_str()); delete b; return nullptr; } while (0)
            HxParams p;
            if (!hx_resolve(c, &p)) {
                // (a limit of this library's layout is named as such: the reference would have taken the configuration)
                if (*hx_resolve_error()) REFUSE_ENTRY(std::string("configuration rejected: ") + hx_resolve_error());
                REFUSE_ENTRY("configuration rejected (the reference's L3_audio_encode_init returns 0 for it)");
            }
            if (p.filter_dc) b->any_dc = true;
            if (b->params.empty()) { b->nchan = p.nchan; b->lsf = p.h_id ? 0 : 1; b->alloc1 = p.alloc1; }
            else if (names.any) { if (!p.h_id) b->lsf = 1; }     // (any kind beside any other: hx_batch::kinds)
            else if (p.alloc1 != b->alloc1) REFUSE_ENTRY("intensity-stereo / dual-channel streams (first-generation allocator) cannot share a batch with the others");
            else if (p.nchan != b->nchan && !names.mixed) REFUSE_ENTRY("mono and stereo streams cannot share a batch (the PCM layout differs)");
            else if ((p.h_id ? 0 : 1) != b->lsf) REFUSE_ENTRY("MPEG-1 and MPEG-2 sample rates cannot share a batch (frames per call differ)");
            if (p.nchan > b->nchan) b->nchan = p.nchan;         // (a mixed menu: the rows are pitched for its widest entry)
            seen.push_back(*c);
            b->params.push_back(p);
            b->cls_kind.push_back(2 * (p.alloc1 ? 1 : 0) + (p.h_id ? 0 : 1));
            b->kinds |= 1u << b->cls_kind.back();
            k = (int) seen.size() - 1;
        }
        b->menu_cls[j] = k;
        // (what src_encode_control derived and what the plan was made for are one decision: a difference is this library's error)
        if (src && plans[menu_plan[j]].nch != b->params[k].nchan) {
            const std::string pre = entry_prefix(names.cls_label, names.origin, j);
            REFUSE_ENTRY("a converter's output channels differ from its encode control's");
        }
    }
#undef REFUSE_ENTRY
    for (int s = 0; s < nstreams; s++) { b->cfg_of[s] = cfg ? cfg[s] : 0; b->cls_of[s] = b->menu_cls[b->cfg_of[s]]; }
    // the device, once the menu stands (nothing of the batch is on it yet: a refusal here only drops the host record)
#define REFUSE_DEVICE(...) do { set_err(__VA_ARGS__); delete b; return nullptr; } while (0)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) REFUSE_DEVICE("no HIP device available: the encoder has no CPU fallback");
    if (device < 0 || device >= ndev) REFUSE_DEVICE("device index out of range");
    {   // written for gfx950 (MI355X) only: the code object holds no other target
        hipDeviceProp_t prop;
        const hipError_t e = hipGetDeviceProperties(&prop, device);
        if (e != hipSuccess) REFUSE_DEVICE("HIP error: %s", hipGetErrorString(e));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) REFUSE_DEVICE("device is %s: this library runs on gfx950 (MI355X) only", prop.gcnArchName);
    }
    // the launch bookkeeping (streams x granules x 9 energies per channel) is 32-bit
    if ((long long) nstreams * max_frames > 32LL * 1024 * 1024) REFUSE_DEVICE("nstreams * max_frames exceeds 32 Mi frames per call: split the batch");
    {
        const hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) REFUSE_DEVICE("HIP error: %s", hipGetErrorString(e));
    }
#undef REFUSE_DEVICE
    b->ncls = (int) b->params.size();
    const long long S = nstreams, NG = 2LL * max_frames;
    std::vector<HxGlobalTabs> gt_host(1);       // (144 KB: not on the stack)
    HxGlobalTabs &gt = gt_host[0];
    hx_global_tabs(&gt);
    std::vector<HxStream> st(nstreams);
    for (int s = 0; s < nstreams; s++) hx_stream_reset(&b->params[b->cls_of[s]], b->cls_of[s], &st[s]);
#define ALLOC(ptr, bytes) do { if (dev_alloc(b, ptr, bytes) != 0) { hx_batch_destroy(b); return nullptr; } } while (0)
    ALLOC(b->d_prm, sizeof(HxParams) * b->ncls + 256);        // (k_spec reads a spreading row in 16-byte pieces, up to 60 bytes past its end)
    ALLOC(b->d_gt, sizeof(HxGlobalTabs));
    ALLOC(b->d_st, sizeof(HxStream) * S);
    ALLOC(b->d_sb, sizeof(float) * S * 2 * (NG + 3) * 576);
    ALLOC(b->d_lens, sizeof(int) * 4 * S);
    if (alloc_set(b, 0) != 0) { hx_batch_destroy(b); return nullptr; }
    ALLOC(b->d_eng, sizeof(int) * S * 2 * NG * 9);
    ALLOC(b->d_flg, S * NG);
    ALLOC(b->d_status, sizeof(int));
    ALLOC(b->d_outbytes, sizeof(int) * S);
    if (const char *e = getenv("HMP3AMD_LPT")) b->lpt = atoi(e);
    if (const char *e = getenv("HMP3AMD_EXACT_SUMS")) b->strict_sums = atoi(e) != 0;
    if (const char *e = getenv("HMP3AMD_PARK_PAIR")) b->park_pair = atoi(e) != 0;
    if (const char *e = getenv("HMP3AMD_PARK")) { b->park_k = atoi(e); if (b->park_k < 0) b->park_k = 0; if (b->park_k > HX_PARK_MAX) b->park_k = HX_PARK_MAX; }
    ALLOC(b->d_dur, sizeof(unsigned) * 2 * S);        // [S] durations, [S] where workgroup i of the last launch ran (see "place")
    ALLOC(b->d_order, sizeof(int) * S);
    HIPCHKN(hipMemset(b->d_dur, 0, sizeof(unsigned) * 2 * S));
    ALLOC(b->d_done, HX_CNT_WORDS * sizeof(int));
    HIPCHKN(hipMemset(b->d_done, 0, HX_CNT_WORDS * sizeof(int)));
    {
        hipDeviceProp_t prop;
        int per_cu = 0;
        HIPCHKN(hipGetDeviceProperties(&prop, device));
        // (of a batch of several kinds: the resident set of its first kind's kernel - what the gates, the launch order's rule
        // and the choice below count in; the kernels' footprints differ by little)
        const void *const walk[4] = {(const void *) k_alloc, (const void *) k_alloc_lsf, (const void *) k_alloc1, (const void *) k_alloc1_lsf};
        const bool kind0 = (b->kinds & 1u) != 0;
        const void *kern = walk[__builtin_ctz(b->kinds)];
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 128, 0) != hipSuccess || per_cu <= 0) per_cu = 4;
        b->resident = per_cu * prop.multiProcessorCount;
        b->ncu = prop.multiProcessorCount;
        // Two builds of the MPEG-1 stream walk.  A batch that the chip holds at once (config 2: 1024 streams on 256 CUs x 4)
        // runs the one written for 256 registers and 38 KB of LDS per stream; a larger one runs k_alloc_slim, whose streams
        // take 168 registers and 26.5 KB, six to a CU: a stream is slower there, 1.5 x as many are in flight.
        // HMP3AMD_K6 = fat | slim overrides the choice (tests run every case on both).
        // (the choice is the kind-0 streams': the other kinds have one kernel each)
        bool slim_ok = kind0;
        for (int k = 0; k < b->ncls && slim_ok; k++) if (b->cls_kind[k] == 0) slim_ok = hx_slim_tables_ok(&b->params[k], &gt) != 0;
        const char *e = getenv("HMP3AMD_K6");
        if (e && strcmp(e, "slim") != 0 && strcmp(e, "fat") != 0) { set_err("HMP3AMD_K6 must be 'fat' or 'slim'"); hx_batch_destroy(b); return nullptr; }
        const bool want = e ? (strcmp(e, "slim") == 0) : (S > b->resident);
        if (e && strcmp(e, "slim") == 0 && !slim_ok && kind0) { set_err("HMP3AMD_K6=slim: the host's tables do not have the structure k_alloc_slim derives them from"); hx_batch_destroy(b); return nullptr; }
        if (want && slim_ok) {
            b->slim = 1;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *) k_alloc_slim, 128, 0) != hipSuccess || per_cu <= 0) per_cu = 6;
            b->resident = per_cu * prop.multiProcessorCount;
        }
    }
    if (b->any_dc) ALLOC(b->d_pcmf, sizeof(float) * S * max_frames * 1152 * b->nchan);
    HIPCHKN(hipMemcpy(b->d_prm, b->params.data(), sizeof(HxParams) * b->ncls, hipMemcpyHostToDevice));
    HIPCHKN(hipMemcpy(b->d_gt, &gt, sizeof(gt), hipMemcpyHostToDevice));
    HIPCHKN(hipMemcpy(b->d_st, st.data(), sizeof(HxStream) * S, hipMemcpyHostToDevice));
    if (slots_init(b) != 0) { hx_batch_destroy(b); return nullptr; }
    HIPCHKN(hipMemset(b->d_sb, 0, sizeof(float) * S * 2 * (NG + 3) * 576));
    HIPCHKN(hipMemset(b->d_status, 0, sizeof(int)));
    b->lastNG = 0;
    if (src && src_setup(b, plans) != 0) { hx_batch_destroy(b); return nullptr; }
    return b;
}

extern "C" hx_batch *hx_batch_create_menu(int device, int nstreams, const HX_E_CONTROL *ec, int nmenu, const HX_SOURCE *src, const int *cfg, int max_frames)
{
    return batch_create(device, nstreams, ec, nmenu, src, cfg, max_frames, MenuNames{"menu entry", "menu entry", nullptr});
}
// the menu of a batch created from per-stream controls: the distinct ones, in order of first appearance
extern "C" hx_batch *hx_batch_create(int device, int nstreams, const HX_E_CONTROL *ec, int shared_control, int max_frames)
{
    if (nstreams <= 0 || max_frames <= 0 || !ec) { set_err("bad arguments"); return nullptr; }
    if (shared_control) return batch_create(device, nstreams, ec, 1, nullptr, nullptr, max_frames, MenuNames{nullptr, nullptr, nullptr});
    std::vector<HX_E_CONTROL> menu;
    std::vector<int> cfg(nstreams);
    for (int s = 0; s < nstreams; s++) {
        int k = -1;
        for (size_t i = 0; i < menu.size(); i++) if (memcmp(&menu[i], ec + s, sizeof(HX_E_CONTROL)) == 0) { k = (int) i; break; }
        if (k < 0) { menu.push_back(ec[s]); k = (int) menu.size() - 1; }
        cfg[s] = k;
    }
    return batch_create(device, nstreams, menu.data(), (int) menu.size(), nullptr, cfg.data(), max_frames, MenuNames{nullptr, nullptr, nullptr});
}

// ... whose entries may differ in channel count
extern "C" hx_batch *hx_batch_create_mixed(int device, int nstreams, const HX_E_CONTROL *ec, int nmenu, const HX_SOURCE *src, const int *cfg, int max_frames)
{
    return batch_create(device, nstreams, ec, nmenu, src, cfg, max_frames, MenuNames{"menu entry", "menu entry", nullptr, true});
}
// ... and in MPEG version and allocator generation
extern "C" hx_batch *hx_batch_create_any(int device, int nstreams, const HX_E_CONTROL *ec, int nmenu, const HX_SOURCE *src, const int *cfg, int max_frames)
{
    return batch_create(device, nstreams, ec, nmenu, src, cfg, max_frames, MenuNames{"menu entry", "menu entry", nullptr, true, true});
}
extern "C" int hx_batch_pcm_channels(const hx_batch *b) { return b ? b->nchan : 0; }
extern "C" int hx_batch_stream_frames_per_block(const hx_batch *b, int i) { return (b && i >= 0 && i < b->S) ? frames_per_block(b->params[b->cls_of[i]]) : -1; }
extern "C" int hx_batch_stream_channels(const hx_batch *b, int i) { return (b && i >= 0 && i < b->S) ? b->params[b->cls_of[i]].nchan : -1; }

extern "C" int hx_batch_nconfigs(const hx_batch *b) { return b ? (int) b->menu_cls.size() : 0; }
extern "C" int hx_batch_stream_config(const hx_batch *b, int i) { return (b && i >= 0 && i < b->S) ? b->cfg_of[i] : -1; }

extern "C" int hx_batch_nstreams(const hx_batch *b) { return b ? b->S : 0; }

extern "C" long long hx_batch_out_stride(const hx_batch *b, int nframes)
{
    if (!b) return 0;
    // nframes new frames plus the images of the frames still pending from earlier calls (their
    // free space is at most the 511-byte reservoir, so a handful of frames; 4 KB covers them)
    // (over the menu's classes, each with its own frames per block: a menu of one MPEG version takes its largest frame)
    long long n = 0;
    for (const HxParams &p : b->params) {
        const int fb = p.vbr_flag ? p.vbr_framebytes[p.ivbr_max] : p.framebytes + 1;
        n = std::max(n, (long long) (frames_per_block(p) * nframes + 2) * fb + 4096);
    }
    return (n + 255) & ~255LL;
}

extern "C" void hx_batch_packet_buffers(hx_batch *b, unsigned char *d_packet, long long frame_stride, int *d_packet_bytes)
{
    b->opt.packet = d_packet; b->opt.packet_stride = frame_stride; b->opt.packet_bytes = d_packet_bytes;
}

extern "C" void hx_batch_frame_stats_buffer(hx_batch *b, int *d_stats) { b->opt.frame_stats = d_stats; }

extern "C" int hx_batch_crc_buffer(hx_batch *b, unsigned short *d_crc)
{
    if (!b) { set_err("null batch"); return -1; }
    if (((unsigned long long) d_crc & 1) != 0) { set_err("d_crc must be 2-byte aligned"); return -1; }
    b->opt.crc = d_crc;
    return 0;
}

// Decoded PCM (include/hmp3_amd.h, "decoded PCM"; kernels: hx_recon.hip).  recon_refused: a menu with a class of another kind
// than 0 - the frame record that gives the kernels their side information holds, for an MPEG-2 block, only the second frame's
// ms (hx_alloc3.inc, place_frame: the (!LSF || part) write), and the first-generation allocator's intensity positions are not
// in it at all.  recon_reserve: everything the output needs on the device, made once and kept; the carried state starts at zero.
int recon_refused(const hx_batch *b)
{
    if (!b) { set_err("null batch"); return -1; }
    for (size_t c = 0; c < b->params.size(); c++)
        if (b->cls_kind[c] != 0) {
            const HxParams &p = b->params[c];
            char msg[256];
            snprintf(msg, sizeof msg, "decoded PCM covers MPEG-1 streams of the second-generation allocator only: class %d of the batch (%d Hz, mode %d%s) is %s",
                     (int) c, p.samprate, p.h_mode, p.is_flag ? ", intensity stereo" : "", p.h_id ? "coded by the first-generation allocator" : "an MPEG-2 rate");
            set_err("%s", msg);
            return -1;
        }
    return 0;
}
int recon_reserve(hx_batch *b)
{
    if (recon_refused(b) != 0) return -1;
    if (b->d_recon_state) return 0;
    int dev0 = -1;
    HIPCHK(hipGetDevice(&dev0));
    HIPCHK(hipSetDevice(b->device));
    const long long S = b->S, NG = 2LL * b->maxF;
    HxReconTabs *t = new HxReconTabs;
    HxGlobalTabs *g = new HxGlobalTabs;
    hx_global_tabs(g);
    hx_recon_tabs(t, g);
    float *state = nullptr;
    int rc = -1;
    // (the state last: it is what says that everything is there; a call that fails half way leaves the rest to hx_batch_destroy)
    if (drain(b) == 0 && dev_alloc(b, b->d_recon_tabs, sizeof(HxReconTabs)) == 0 && dev_alloc(b, b->d_recon_hyb, sizeof(float) * S * NG * 1152) == 0 &&
        dev_alloc(b, b->d_recon_tails, sizeof(float) * S * HX_RECON_TAIL_FLOATS) == 0 &&
        (b->walk[0].rec || dev_alloc(b, b->walk[0].rec, sizeof(HxFrameDebug) * S * b->maxF) == 0) &&
        (!b->walk[1].ixq || b->walk[1].rec || dev_alloc(b, b->walk[1].rec, sizeof(HxFrameDebug) * S * b->maxF) == 0) &&
        dev_alloc(b, state, sizeof(float) * S * HX_RECON_STATE_FLOATS) == 0 &&
        hipMemcpy(b->d_recon_tabs, t, sizeof(HxReconTabs), hipMemcpyHostToDevice) == hipSuccess &&
        hipMemset(state, 0, sizeof(float) * S * HX_RECON_STATE_FLOATS) == hipSuccess && hipDeviceSynchronize() == hipSuccess) {
        b->d_recon_state = state;
        rc = 0;
    } else if (!b->poisoned && rc != 0) set_err("decoded PCM: the device buffers could not be made");
    delete t;
    delete g;
    (void) hipSetDevice(dev0);
    return rc;
}
extern "C" int hx_batch_recon_buffer(hx_batch *b, float *d_recon)
{
    if (!b) { set_err("null batch"); return -1; }
    if (!d_recon) { b->opt.recon = nullptr; return 0; }
    if (((unsigned long long) d_recon & 3) != 0) { set_err("d_recon must be 4-byte aligned"); return -1; }
    if (check_poisoned(b) != 0 || recon_reserve(b) != 0) return -1;
    b->opt.recon = d_recon;
    return 0;
}
extern "C" int hx_recon_delay(void) { return 2209; }

// Per-stream frame counts of the calls that follow.  Only the host copy changes here: a call checks it against its nframes
// (check_args) and uploads it for itself (encode_pass), so what is set later never reaches a call already made.
// counts_reserve: everything that can fail - whether the batch takes counts at all, and (buffers) at the first use their
// staging (staging_make).  The calling thread's current device is left as it was.
// counts_buffers: the second part alone - a converting batch, which the setter refuses, takes its counts as an argument of
// hx_batch_encode_src_counts_* and needs the same staging.
int counts_reserve(hx_batch *b, bool buffers)
{
    if (!b) { set_err("null batch"); return -1; }
    if (b->nsrc) { set_err("a converting batch takes its per-stream frame counts per call, not from this setter: hx_batch_encode_src_counts_*"); return -1; }
    return buffers ? counts_buffers(b) : 0;
}
int counts_buffers(hx_batch *b)
{
    if (b->nfr_stage.d) return 0;
    int dev0 = -1;
    HIPCHK(hipGetDevice(&dev0));
    HIPCHK(hipSetDevice(b->device));
    const int rc = staging_make(b, b->nfr_stage, sizeof(int) * (size_t) b->S);
    (void) hipSetDevice(dev0);
    return rc;
}
extern "C" int hx_batch_frame_counts(hx_batch *b, const int *nfr)
{
    if (counts_reserve(b, nfr != nullptr) != 0) return -1;
    if (nfr) b->nfr.assign(nfr, nfr + b->S);
    else b->nfr.clear();
    return 0;
}

// PCM segments of the calls that follow.  Like the counts, only the host copy changes here: a call checks it against its
// nframes, its sample size and the counts and channels as of the call (check_segments) and uploads it for itself
// (upload_image), so what is set later never reaches a call already made.
extern "C" long long hx_pcm_packed_layout(int nstreams, int nframes, const int *nfr, const int *channels, int sample_bytes, long long *off)
{
    if (nstreams < 0 || nframes < 0 || !off || !channels || (sample_bytes != 2 && sample_bytes != 4)) return -1;
    for (int i = 0; i < nstreams; i++)
        if ((channels[i] != 1 && channels[i] != 2) || (nfr && (nfr[i] < 0 || nfr[i] > nframes))) return -1;
    off[0] = 0;
    for (int i = 0; i < nstreams; i++) off[i + 1] = off[i] + (long long) (nfr ? nfr[i] : nframes) * 1152 * channels[i] * sample_bytes;
    return off[nstreams];
}
int segs_reserve(hx_batch *b, bool buffers)
{
    if (!b) { set_err("null batch"); return -1; }
    if (b->nsrc) { set_err("a converting batch takes no PCM segments: its input is per stream already (in_stride, frame_off)"); return -1; }
    if (!buffers || b->img_stage.d) return 0;
    int dev0 = -1;
    HIPCHK(hipGetDevice(&dev0));
    HIPCHK(hipSetDevice(b->device));
    const int rc = staging_make(b, b->img_stage, planes_stage_bytes(b));       // (the wider of the two layouts)
    (void) hipSetDevice(dev0);
    return rc;
}
extern "C" int hx_batch_pcm_segments(hx_batch *b, const long long *off, long long in_bytes)
{
    if (segs_reserve(b, off != nullptr) != 0) return -1;
    if (off && in_bytes < 0) { set_err("in_bytes < 0"); return -1; }
    if (off) { b->seg_off.assign(off, off + b->S); b->seg_bytes = in_bytes; }
    else { b->seg_off.clear(); b->seg_bytes = 0; }
    b->pl_off.clear(); b->pl_stride.clear(); b->pl_bytes = 0; b->pl_unit = false;       // (segments and planes exclude each other)
    return 0;
}
int check_segments(const hx_batch *b, int nframes, int sample_bytes, int first)
{
    if (!b || b->seg_off.empty()) return 0;
    for (int i = 0; i < b->S; i++) {
        const long long n = seg_len(b, i, nframes, sample_bytes), o = b->seg_off[i];
        if (n <= 0) continue;
        const char *what = o < 0 ? "is negative" : (o % sample_bytes) != 0 ? "is no multiple of the call's sample size" :
                           (n > b->seg_bytes || o > b->seg_bytes - n) ? "ends beyond in_bytes" : nullptr;
        if (what) {
            char msg[192];
            snprintf(msg, sizeof msg, "stream %d: PCM segment at offset %lld (%lld bytes, in_bytes = %lld) %s", first + i, o, n, b->seg_bytes, what);
            set_err("%s", msg);
            return -1;
        }
    }
    return 0;
}

// PCM planes of the calls that follow: segments' sibling (include/hmp3_amd.h, "PCM planes").  Only the host copy changes
// here; a call checks it (check_planes) and uploads offsets and strides for itself (upload_image).
extern "C" long long hx_pcm_planar_layout(int nstreams, int nframes, const int *nfr, const int *channels, int sample_bytes, long long *off,
                                          long long *chan_stride)
{
    if (nstreams < 0 || nframes < 0 || !off || !chan_stride || !channels || (sample_bytes != 2 && sample_bytes != 4)) return -1;
    for (int i = 0; i < nstreams; i++)
        if ((channels[i] != 1 && channels[i] != 2) || (nfr && (nfr[i] < 0 || nfr[i] > nframes))) return -1;
    off[0] = 0;
    for (int i = 0; i < nstreams; i++) {
        chan_stride[i] = (long long) (nfr ? nfr[i] : nframes) * 1152 * sample_bytes;
        off[i + 1] = off[i] + chan_stride[i] * channels[i];
    }
    return off[nstreams];
}
int planes_args(const long long *off, long long in_bytes, int unit_scale)
{
    if (off && in_bytes < 0) { set_err("in_bytes < 0"); return -1; }
    if (off && unit_scale != 0 && unit_scale != 1) { set_err("unit_scale must be 0 (int16 scale) or 1 (x * 32768.0f)"); return -1; }
    return 0;
}
extern "C" int hx_batch_pcm_planes(hx_batch *b, const long long *off, const long long *chan_stride, long long in_bytes, int unit_scale)
{
    if (segs_reserve(b, off != nullptr) != 0 || planes_args(off, in_bytes, unit_scale) != 0) return -1;
    b->seg_off.clear(); b->seg_bytes = 0;               // (segments and planes exclude each other)
    b->pl_off.clear(); b->pl_stride.clear(); b->pl_bytes = 0; b->pl_unit = false;
    if (!off) return 0;
    b->pl_off.assign(off, off + b->S);
    if (chan_stride) b->pl_stride.assign(chan_stride, chan_stride + b->S);
    b->pl_bytes = in_bytes; b->pl_unit = unit_scale == 1;
    return 0;
}
int check_planes(const hx_batch *b, int nframes, int sample_bytes, int first)
{
    if (!b || b->pl_off.empty()) return 0;
    if (b->pl_unit && sample_bytes != 4) { set_err("an s16 call under PCM planes with unit_scale = 1: unit scale is defined for fp32 samples only"); return -1; }
    for (int i = 0; i < b->S; i++) {
        const long long n = plane_len(b, i, nframes, sample_bytes), d = plane_stride(b, i, nframes, sample_bytes);
        if (n <= 0) continue;
        for (int c = 0; c < b->params[b->cls_of[i]].nchan; c++) {
            // (offset and stride are the caller's: a sum that leaves the i64 range is refused like any other start outside the image)
            long long o = 0;
            const bool wild = __builtin_add_overflow(b->pl_off[i], c * d, &o);
            const char *what = wild ? "lies outside the image" : o < 0 ? "starts below 0" : (o % sample_bytes) != 0 ? "is no multiple of the call's sample size" :
                               (n > b->pl_bytes || o > b->pl_bytes - n) ? "ends beyond in_bytes" : nullptr;
            if (what) {
                char msg[224];
                snprintf(msg, sizeof msg, "stream %d channel %d: PCM plane at offset %lld (%lld bytes, in_bytes = %lld) %s", first + i, c, o, n, b->pl_bytes, what);
                set_err("%s", msg);
                return -1;
            }
        }
    }
    return 0;
}

extern "C" long long hx_batch_dense_bound(const hx_batch *b, int nframes)
{
    return b ? (long long) b->S * ((hx_batch_out_stride(b, nframes) + 15) & ~15LL) : 0;
}

extern "C" int hx_batch_dense_buffers(hx_batch *b, unsigned char *d_dense, long long dense_cap, long long *d_dense_off)
{
    if (!b) { set_err("null batch"); return -1; }
    if (!d_dense) { b->opt.dense = DenseOut(); return 0; }
    if (((unsigned long long) d_dense & 15) != 0) { set_err("d_dense must be 16-byte aligned"); return -1; }
    if (!d_dense_off || ((unsigned long long) d_dense_off & 7) != 0 || dense_cap < 0) { set_err("d_dense_off must be an array of nstreams + 1 long long and dense_cap >= 0"); return -1; }
    b->opt.dense = DenseOut{d_dense, dense_cap, d_dense_off, nullptr};
    return 0;
}

extern "C" void hx_batch_debug_enable(hx_batch *b, int on)
{
    b->debug = on != 0;
    if (on && !b->d_dbg) {
        hipSetDevice(b->device);
        dev_alloc(b, b->d_dbg, sizeof(HxFrameDebug) * (size_t) b->S * b->maxF);
        dev_alloc(b, b->d_xrdbg, sizeof(float) * (size_t) b->S * 2 * b->maxF * 1152);
        dev_alloc(b, b->d_dbgmetric, sizeof(int) * (size_t) b->S * 2 * b->maxF * 4);      // k_detect's metrics: a0, b0, a1, b1 per granule
        if (dev_alloc(b, b->d_prof, sizeof(unsigned long long) * (size_t) b->S * HX_PROF_WORDS) == 0) hipMemset(b->d_prof, 0, sizeof(unsigned long long) * (size_t) b->S * HX_PROF_WORDS);
    }
}

// streams, events and the second buffer set of the submit path, created at the first submit
static int pipe_init(hx_batch *b)
{
    if (b->s_front) return 0;
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));          // lo = least urgent, hi = most urgent
    if (new_stream(b, b->s_front, lo) || new_stream(b, b->s_alloc, hi) || new_stream(b, b->s_pack, lo) || new_event(b, b->ev_in)) return -1;
    for (int i = 0; i < 2; i++)
        if (new_event(b, b->ev_front[i]) || new_event(b, b->ev_alloc[i]) || new_event(b, b->ev_k6[i])) return -1;
    for (int i = 0; i < 3; i++) if (new_event(b, b->ev_sgn[i])) return -1;
    return alloc_set(b, 1);
}

int check_poisoned(const hx_batch *b)
{
    if (b->poisoned) { set_err("the batch is unusable after a failed device call: destroy it"); return -1; }
    return 0;
}
// outputs = false (the *_host_files calls): the call has no output buffers of the caller's, `out` and `out_bytes` are not looked at
int check_args(const hx_batch *b, const void *in, int nframes, const void *out, long long out_stride, const void *out_bytes, bool outputs)
{
    if (!b) { set_err("null batch"); return -1; }
    if (check_poisoned(b) != 0) return -1;
    if (nframes <= 0 || nframes > b->maxF) { set_err("nframes out of range (1 .. max_frames of hx_batch_create)"); return -1; }
    if (!in || (outputs && (!out || !out_bytes))) { set_err("null buffer"); return -1; }
    if (out_stride < hx_batch_out_stride(b, nframes)) { set_err("out_stride is smaller than hx_batch_out_stride(b, nframes)"); return -1; }
    return check_counts(b, nframes, 0);
}
// (hx_batch_frame_counts: a count no kernel could honour never reaches one)
int check_counts(const hx_batch *b, int nframes, int first)
{
    return check_counts_arg(b->nfr.data(), (int) b->nfr.size(), nframes, first);
}
int check_counts_arg(const int *nfr, int S, int nframes, int first)
{
    for (int i = 0; nfr && i < S; i++)
        if (nfr[i] < 0 || nfr[i] > nframes) {
            char msg[96];
            snprintf(msg, sizeof(msg), "stream %d: frame count %d out of range (0 .. nframes = %d)", first + i, nfr[i], nframes);
            set_err("%s", msg);
            return -1;
        }
    return 0;
}
// (k_crc takes every e[f] from the call's frame counters, and the batch keeps no counter buffer of its own for it: two
// pipelined submits would race on one)
// (k_ledger takes a live record's end, bytes and CRC from the call's counters and CRCs: the same rule, for both buffers)
int check_opt(const hx_batch *b, const OptOut &o, const int *nfr, int first)
{
    if (o.crc && !o.frame_stats) { set_err("a CRC buffer (hx_batch_crc_buffer) needs a frame-counter buffer (hx_batch_frame_stats_buffer) in force"); return -1; }
    if (!b || !b->d_ledger || (o.crc && o.frame_stats)) return 0;
    for (int s = 0; s < b->S; s++)
        if (b->led_live[s] && (!nfr || nfr[s] > 0)) {
            char msg[192];
            snprintf(msg, sizeof msg, "stream %d has an open ledger record (hx_batch_ledger_begin): a call that feeds it needs a frame-counter buffer and a CRC buffer in force", first + s);
            set_err("%s", msg);
            return -1;
        }
    return 0;
}
// (a converting batch takes its input through hx_batch_encode_src_* only: a plain call would advance the encoder past its converter)
int check_call(const hx_batch *b, const void *pcm, int nframes, const void *out, long long out_stride, const void *out_bytes, bool outputs)
{
    if (b && b->nsrc) { set_err("a converting batch takes its input through hx_batch_encode_src_*"); return -1; }
    return check_args(b, pcm, nframes, out, out_stride, out_bytes, outputs);
}

// k_pack over every frame position of a call on stream qp (solo 0: the packing alone): the grid fills the chip once, a
// workgroup takes every gridDim.x-th position (hx_pack.hip).  The one launch expression: a batch's call and hx_debug_pack.
static int launch_pack(hipStream_t qp, const HxStream *st, const HxParams *prm, const HxGlobalTabs *gt, const short *ixq, const unsigned *sgn,
                       const HxSegOut *seg, const HxFrameOut *frm, const HxSlot *slots, unsigned char *out, long long out_stride,
                       unsigned char *packet, int *status, int fps, int NG, long long total, const int *nfr)
{
    LAUNCH(k_pack, dim3((unsigned) (total < 8LL * 256 * 8 ? total : 8LL * 256 * 8)), dim3(256), qp, st, prm, gt, ixq, sgn, seg, frm, slots,
           out, out_stride, packet, status, fps, NG, total, 0, (HxStream *) nullptr, (const int *) nullptr, (const int *) nullptr, (const int *) nullptr, (unsigned *) nullptr, (unsigned char *) nullptr, (const int *) nullptr, nfr);
    return 0;
}

// the packing kernels of one call on stream qp (see place_pack)
static int enqueue_pack(hx_batch *b, const Call &c, int nframes, int set, int sset, hipStream_t qp)
{
    const int S = b->S, NG = 2 * nframes;
    const WalkSet &w = b->walk[set];
    const unsigned *sgn = b->sgn[sset];
    const int fps = (b->lsf ? 2 : 1) * nframes;      // frame positions per stream = the records' stride (AllocArgs::fpc)
    const long long total = (long long) S * fps;
    // a handful of frames in all (the one-stream encoder's calls): one workgroup does the three kernels' work (hx_pack.hip, solo)
    const int solo = (S <= 4 && total <= 8) ? S : 0;
    if (solo) {
        LAUNCH(k_pack, dim3(1), dim3(256), qp, b->d_st, b->d_prm, b->d_gt, w.ixq, sgn, w.seg, w.frm, w.slots,
               c.out, c.out_stride, c.opt.packet, b->d_status, fps, NG, total, solo, b->d_st, w.pre_len, c.out_bytes, w.carry_len, c.rec_frames,
               (solo == 1) ? c.rec_host : (unsigned char *) nullptr, b->d_done + HX_CNT_STARTED, c.nfr);
        return 0;
    }
    LAUNCH(k_pack_pre, dim3(S), dim3(64), qp, b->d_st, c.out, c.out_stride, w.pre_len);
    if (launch_pack(qp, b->d_st, b->d_prm, b->d_gt, w.ixq, sgn, w.seg, w.frm, w.slots, c.out, c.out_stride, c.opt.packet, b->d_status, fps, NG, total, c.nfr) != 0) return -1;
    LAUNCH(k_pack_carry, dim3(S), dim3(64), qp, b->d_st, c.out, c.out_stride, c.out_bytes, w.carry_len, c.rec_frames);
    return 0;
}

// the dense image of one call on stream qp, right behind its packing kernels (hx_pack.hip): offsets, then the gather over
// (stream, chunk of the worst-case row)
static int enqueue_dense(hx_batch *b, const Call &c, int nframes, hipStream_t qp)
{
    const DenseOut &d = c.opt.dense;
    if (!d.buf) return 0;
    const int chunks = (int) ((hx_batch_out_stride(b, nframes) + HX_DENSE_CHUNK - 1) / HX_DENSE_CHUNK);
    LAUNCH(k_dense_off, dim3(1), dim3(1024), qp, c.out_bytes, d.off, d.off_copy, b->S, d.cap, b->d_status);
    LAUNCH(k_dense_gather, dim3((unsigned) ((long long) b->S * chunks)), dim3(256), qp, c.out, c.out_stride, c.out_bytes, (const long long *) d.off, d.buf, d.cap, chunks);
    return 0;
}

// the per-frame MusicCRC of one call on stream qp, behind its packing (hx_crc.hip): one workgroup per stream
static int enqueue_crc(hx_batch *b, const Call &c, int nframes, hipStream_t qp)
{
    if (!c.opt.crc) return 0;
    LAUNCH(k_crc, dim3(b->S), dim3(256), qp, c.out, c.out_stride, c.out_bytes, (const int *) c.opt.frame_stats, nframes, c.opt.crc);
    return 0;
}

// The frame records a pass's stream walk writes (AllocArgs::dbg) and its decoded-PCM kernels read: the debug taps' array, or -
// with the decoded PCM on - the buffer set's own, so that a deferred packing reads what its own walk wrote.  With both on, a
// plain call's records go to the taps' array and serve both; a submit's go to its set's own array, so the "dbg" tap is not
// written for a submit made with the decoded PCM on (include/hmp3_amd.h says so).
static HxFrameDebug *frame_records(const hx_batch *b, const Call &c, int set, PassKind kind)
{
    if (b->debug && (kind == PASS_PLAIN || !c.opt.recon)) return b->d_dbg;
    return c.opt.recon ? b->walk[set].rec : nullptr;
}
// The decoded PCM of S streams x NG granule positions on stream qp (hx_recon.hip): the hybrid over (stream, granule), the
// synthesis over (stream, frame), then the carried state per stream.  The one launch expression: a batch's call and hx_debug_recon.
static int launch_recon(hipStream_t qp, const HxStream *st, const HxParams *prm, const HxGlobalTabs *gt, const HxReconTabs *rt, const short *ixq,
                        const unsigned *sgn, const HxSegOut *seg, const HxFrameDebug *rec, float *hyb, float *tails, float *state, float *out,
                        long long row, int S, int NG, const int *nfr)
{
    const dim3 grid((unsigned) ((long long) S * NG));
    LAUNCH(k_recon_hybrid, grid, dim3(256), qp, st, prm, gt, rt, ixq, sgn, seg, rec, hyb, tails, (const float *) state, NG, nfr);
    LAUNCH(k_recon_synth, dim3((unsigned) ((long long) S * (NG / 2))), dim3(256), qp, st, prm, rt, (const float *) hyb, (const float *) state, out, row, NG, nfr);
    LAUNCH(k_recon_carry, dim3(S), dim3(256), qp, st, prm, (const float *) hyb, (const float *) tails, state, NG, nfr);
    return 0;
}
// the decoded PCM of one call on stream qp, behind its packing
static int enqueue_recon(hx_batch *b, const Call &c, int nframes, int set, int sset, PassKind kind, hipStream_t qp)
{
    if (!c.opt.recon) return 0;
    const WalkSet &w = b->walk[set];
    return launch_recon(qp, (const HxStream *) b->d_st, (const HxParams *) b->d_prm, (const HxGlobalTabs *) b->d_gt, (const HxReconTabs *) b->d_recon_tabs,
                        (const short *) w.ixq, (const unsigned *) b->sgn[sset], (const HxSegOut *) w.seg, (const HxFrameDebug *) frame_records(b, c, set, kind),
                        b->d_recon_hyb, b->d_recon_tails, b->d_recon_state, c.opt.recon, (long long) nframes * 1152 * b->nchan, b->S, 2 * nframes, c.nfr);
}

// the file ledger's update from one call on stream qp, behind its CRC kernel (hx_ledger.hip): one wave per stream.  A call
// made before the batch's first hx_batch_ledger_begin has no ledger in its record
static int enqueue_ledger(hx_batch *b, const Call &c, int nframes, hipStream_t qp)
{
    if (!c.ledger) return 0;
    LAUNCH(k_ledger, dim3((unsigned) ((b->S + 3) / 4)), dim3(256), qp, c.ledger, (const int *) c.opt.frame_stats, (const unsigned short *) c.opt.crc, (const int *) c.out_bytes, c.nfr, nframes, b->S);
    return 0;
}

// the file images' append of one call on stream qp, right behind its ledger update (hx_fileimg.hip): (stream, chunk of the
// worst-case row - plus the 15 bytes a piece may start off a destination vector).  A call without counters and CRCs leaves
// the live records alone (k_ledger), so nothing of it belongs to a file: no launch
static int enqueue_file(hx_batch *b, const Call &c, int nframes, hipStream_t qp)
{
    const FileImages &f = c.files;
    if (!c.ledger || !f.img || !c.opt.frame_stats || !c.opt.crc) return 0;
    const int chunks = (int) ((hx_batch_out_stride(b, nframes) + 15 + HX_FILE_CHUNK - 1) / HX_FILE_CHUNK);
    LAUNCH(k_file_append, dim3((unsigned) ((long long) b->S * chunks)), dim3(256), qp, (const HX_LEDGER *) c.ledger, (uint2 *) f.fw, f.img, f.pitch, f.cap,
           (const unsigned char *) c.out, c.out_stride, c.nfr, nframes, chunks, b->d_status);
    return 0;
}

// A gate on stream q: what follows it there starts in the tail of the allocator launch whose first workgroup took number
// `base` of the started-counter (it wraps with the counter), not at that launch's start.
static int launch_gate(hx_batch *b, hipStream_t q, unsigned base)
{
    if (b->gate_percent <= 0) return 0;
    const long long fill = b->S < b->resident ? b->S : b->resident;     // workgroups of that launch the device holds at once
    LAUNCH(k_gate, dim3(1), dim3(64), q, (const unsigned *) (b->d_done + HX_CNT_STARTED), base, (unsigned) (fill * b->gate_percent / 100), b->d_done + HX_CNT_GATE_TIMEOUTS);
    return 0;
}

// the deferred packing of the latest submit: out now, on the packing stream; gate_base >= 0: behind a gate on the allocator launch
// that was just enqueued (the one after the job's own)
static int flush_pack(hx_batch *b, long long gate_base)
{
    hx_batch::PackJob &j = b->pack_job;
    if (!j.pending) return 0;
    j.pending = false;
    HIPCHK(hipStreamWaitEvent(b->s_pack, b->ev_k6[j.set], 0));
    if (gate_base >= 0 && launch_gate(b, b->s_pack, (unsigned) gate_base) != 0) return -1;
    if (enqueue_pack(b, j.call, j.nframes, j.set, j.sset, b->s_pack) != 0 || enqueue_dense(b, j.call, j.nframes, b->s_pack) != 0 ||
        enqueue_crc(b, j.call, j.nframes, b->s_pack) != 0 || enqueue_ledger(b, j.call, j.nframes, b->s_pack) != 0 ||
        enqueue_file(b, j.call, j.nframes, b->s_pack) != 0 || enqueue_recon(b, j.call, j.nframes, j.set, j.sset, PASS_SUBMIT_DEVICE, b->s_pack) != 0) return -1;
    HIPCHK(hipEventRecord(b->ev_alloc[j.set], b->s_pack));
    HIPCHK(hipEventRecord(b->ev_sgn[j.sset], b->s_pack));
    return 0;
}

// One pass of the pipeline over the batch, as phases in the order they run.  What a phase leaves for the later ones:
struct Pass {
    PcmIn in; int nframes; Call call; PassKind kind;    // the call: the stream walk and the packing write its record's outputs
    hipStream_t q, qa;                  // streams of the front end / of the stream walk and (unless deferred) the packing
    int set = 0, sset = 0;              // buffer set; set of signs (also read by the packing, which may still be busy with
                                        // submit n-2 when the front end of submit n writes them: three sets in rotation)
    int flushed_set = -1;               // the buffer set of a deferred packing that pipe_enter sent out
    const long long *d_img = nullptr;   // under PCM segments: the device copy of the call's offsets, relative to in.p (upload_image);
                                        // under PCM planes: of its offsets and strides, [2][S]
};

int order_behind_submits(hx_batch *b, hipStream_t q)
{
    if (flush_pack(b, -1) != 0) return -1;
    const int last = (int) ((b->nsubmit - 1) & 1);
    HIPCHK(hipStreamWaitEvent(q, b->ev_front[last], 0));
    HIPCHK(hipStreamWaitEvent(q, b->ev_alloc[last], 0));
    return 0;
}

// event ordering on entry: a submit moves to the batch's own streams behind the calls that hold its buffer sets and a
// gate; a plain call behind submits is ordered after them
static int pipe_enter(hx_batch *b, Pass &p)
{
    if (p.kind != PASS_PLAIN) {
        if (pipe_init(b) != 0) return -1;
        if (p.kind == PASS_SUBMIT_HOST && b->pack_job.pending) {    // (a host-buffer submit behind device-buffer ones)
            p.flushed_set = b->pack_job.set;
            if (flush_pack(b, -1) != 0) return -1;
        }
        p.set = (int) (b->nsubmit & 1);
        p.sset = (int) (b->nsubmit % 3);
        HIPCHK(hipEventRecord(b->ev_in, p.q));                      // the caller's PCM is ready from here on
        HIPCHK(hipStreamWaitEvent(b->s_front, b->ev_in, 0));
        if (b->nsubmit >= 2) HIPCHK(hipStreamWaitEvent(b->s_front, b->ev_k6[p.set], 0));      // k_alloc of submit n-2 is done with this set
        if (b->nsubmit >= 3) HIPCHK(hipStreamWaitEvent(b->s_front, b->ev_sgn[p.sset], 0));    // ... and the packing of submit n-3 with this set of signs
        p.q = b->s_front; p.qa = b->s_alloc;
        // (the front end starts in the previous allocator kernel's tail)
        if (b->alloc_launches > 0 && launch_gate(b, p.q, (unsigned) ((unsigned long long) (b->alloc_launches - 1) * (unsigned long long) b->S)) != 0) return -1;
    } else if (b->inflight) {                                       // a plain call behind submits
        if (order_behind_submits(b, p.q) != 0) return -1;
        b->inflight = false;
    }
    return 0;
}

// The call's frame counts to the device: through page-locked staging into copy k of three, on the stream the front end runs
// on (the kernels of the call follow it there or wait for that stream's events).  The staging copy is free when its previous
// upload, three calls ago, is done: the host waits for that here, so a call under counts is not made under stream capture
// and may block behind the call three before it (include/hmp3_amd.h says so).
// Which copy: a submit takes the one of its set of signs - the packing that reads both is done before that set comes round
// again (pipe_enter waits for ev_sgn).  A plain call has no set of signs of its own, so plain calls count their own
// rotation; copy k of a plain call may therefore be the copy of a submit still in flight, and what keeps the upload off
// that submit's kernels is stream order: the upload goes onto the caller's stream behind order_behind_submits (a plain
// call after submits) or, for a submit after plain calls, onto the front-end stream behind ev_in, which is behind
// everything the plain calls put on the caller's stream.
// A converting call has made its upload already, in front of k_src, which reads the same copy (counts_upload_plain: it is a
// plain call, and no submit of a converting batch exists that it could follow): its record arrives with nfr set.
static int counts_upload(hx_batch *b, int k, hipStream_t q, const int *&d_nfr)
{
    Staging &s = b->nfr_stage;
    void *h = staging_take(s, k);
    if (!h) return -1;
    memcpy(h, b->nfr.data(), s.bytes);
    if (staging_upload(s, k, s.bytes, q) != 0 || staging_done(s, k, q) != 0) return -1;
    d_nfr = s.dev<int>(k);
    return 0;
}
int counts_upload_plain(hx_batch *b, hipStream_t q, const int *&d_nfr)
{
    return counts_upload(b, (int) (b->nplain++ % 3), q, d_nfr);
}
static int upload_counts(hx_batch *b, Pass &p)
{
    if (b->nfr.empty() || p.call.nfr) return 0;
    return p.kind == PASS_PLAIN ? counts_upload_plain(b, p.q, p.call.nfr) : counts_upload(b, p.sset, p.q, p.call.nfr);
}

// The call's PCM segments - or its planes' offsets and strides - to the device, like its counts and in their rotation: through page-locked staging into copy k of
// three on the stream the front end runs on, where k_pcm_spread - the only reader - follows.  The same two notes apply: the
// host may wait for the upload of the call three before, and the call is not made under stream capture.  What goes up is
// relative to the pointer the kernel gets (PcmIn::shift); the offset of a stream that takes no frame is not looked at.
static int upload_image(hx_batch *b, Pass &p)
{
    if (!p.in.image()) return 0;
    Staging &s = b->img_stage;
    const int k = p.kind == PASS_PLAIN ? (int) (b->nplain_img++ % 3) : p.sset;
    long long *h = (long long *) staging_take(s, k);
    if (!h) return -1;
    if (p.in.seg)
        for (int i = 0; i < b->S; i++) h[i] = seg_len(b, i, p.nframes, p.in.sample_bytes()) > 0 ? p.in.seg[i] - p.in.shift : 0;
    else    // (planes: the host fills in the stride of a mono stream and of a stream that takes no frame)
        for (int i = 0; i < b->S; i++) {
            h[i] = plane_len(b, i, p.nframes, p.in.sample_bytes()) > 0 ? p.in.pl[i] - p.in.shift : 0;
            h[b->S + i] = plane_stride(b, i, p.nframes, p.in.sample_bytes());
        }
    if (staging_upload(s, k, p.in.seg ? segs_stage_bytes(b) : planes_stage_bytes(b), p.q) != 0 || staging_done(s, k, p.q) != 0) return -1;
    p.d_img = s.dev<long long>(k);
    return 0;
}
// ... and the row buffer of a call under segments or planes, before the pass touches anything: made at the first such call, grown
// behind a drain (an earlier call's front end may still read it)
static int rows_reserve(hx_batch *b, PcmIn in, int nframes)
{
    const long long need = in.bytes(b->S, nframes, b->nchan);
    const long long chunks = (in.bytes(1, nframes, b->nchan) + HX_PCM_CHUNK - 1) / HX_PCM_CHUNK;
    if ((long long) b->S * chunks > INT_MAX) { set_err("nstreams * nframes too large for a call under PCM segments or planes: split the call"); return -1; }
    if (need <= b->rows_cap) return 0;
    HIPCHK(hipSetDevice(b->device));
    if (b->rows_cap > 0 && drain(b) != 0) return -1;
    b->rows_cap = 0;
    if (dev_realloc(b, b->d_rows, need) != 0) return -1;
    b->rows_cap = need;
    return 0;
}

// K4 over S streams x NG granule positions on stream q (hx_spec.hip): one workgroup of two waves per pair of granules,
// in the form that goes with the stream-walk kernel (direct: spec_granule<true>).  sb holds SG subband slots per (stream,
// channel); granule g reads slots g and g + 1.  The one launch expression: a batch's call and hx_debug_spec.
static int launch_spec(hipStream_t q, bool direct, const float *sb, const HxStream *st, const HxParams *prm, const HxGlobalTabs *gt,
                       const unsigned char *bt, float *xr, float *etab, float *thr, int *msbase, int S, int NG, int SG, const int *nfr)
{
    const dim3 grid((unsigned) ((long long) S * (NG / 2)));
    if (direct) LAUNCH(k_spec_direct, grid, dim3(128), q, sb, st, prm, gt, bt, xr, etab, thr, msbase, NG, SG, nfr);
    else LAUNCH(k_spec, grid, dim3(128), q, sb, st, prm, gt, bt, xr, etab, thr, msbase, NG, SG, nfr);
    return 0;
}

// K-1, the head of the front end under segments or planes: k_pcm_spread or k_pcm_planes (hx_pcmin.hip) fills the row buffer
// from the call's image on stream p.q, behind the upload of the image's layout (upload_image).  A call fed rows: nothing.
static int launch_rows(hx_batch *b, const Pass &p)
{
    if (!p.d_img) return 0;
    const int S = b->S, nframes = p.nframes;
    const long long row_bytes = p.in.bytes(1, nframes, b->nchan);
    const int chunks = (int) ((row_bytes + HX_PCM_CHUNK - 1) / HX_PCM_CHUNK);
    const dim3 grid((unsigned) ((long long) S * chunks));
    if (p.in.pl)
        LAUNCH(k_pcm_planes, grid, dim3(256), p.q, (const unsigned char *) p.in.p, p.d_img, S, b->d_rows, row_bytes, nframes, p.in.sample_bytes(), (int) p.in.unit,
               (const HxStream *) b->d_st, (const HxParams *) b->d_prm, p.call.nfr, chunks);
    else
        LAUNCH(k_pcm_spread, grid, dim3(256), p.q, (const unsigned char *) p.in.p, p.d_img, b->d_rows, row_bytes, nframes, p.in.sample_bytes(),
               (const HxStream *) b->d_st, (const HxParams *) b->d_prm, p.call.nfr, chunks);
    b->rows_bytes = row_bytes * S;
    return 0;
}

// the front end: PCM to spectra, psy data and the allocator's start values, into front[set] and sgn[sset]
static int launch_front(hx_batch *b, const Pass &p)
{
    const FrontSet &f = b->front[p.set];
    const hipStream_t q = p.q;
    const int S = b->S, nframes = p.nframes, NG = 2 * nframes;
    const long long nsamp = 1152LL * nframes;
    // under segments or planes: the rows come from K-1 (launch_rows), and the kernels below read them in place of the caller's pointer
    if (launch_rows(b, p) != 0) return -1;
    const void *pcm = p.d_img ? b->d_rows : p.in.p;
    const int16_t *d_pcm = p.in.f32 ? nullptr : (const int16_t *) pcm;
    const float *d_pcm32 = p.in.f32 ? (const float *) pcm : nullptr;
    // The subband carry sits in slots NG_prev..NG_prev+2 only if the previous call used another
    // frame count; k_msscan always rolls it to slots 0..2, so nothing to do here.
    dim3 g1(S, (NG + K1_GPB - 1) / K1_GPB);
    const int SG = 2 * b->maxF + 3;     // subband slots per (stream, channel): fixed layout
    const float *pcmf = b->any_dc ? b->d_pcmf : d_pcm32;       // fp32 samples the polyphase reads, or null for int16
    // (launch dimensions are those of nframes with or without counts: a unit beyond its stream's count does nothing)
    const int *nfr = p.call.nfr;
    if (b->any_dc) LAUNCH(k_dcfilter, dim3((b->nchan * S + 63) / 64), dim3(64), q, d_pcm, d_pcm32, nsamp, b->d_st, b->d_prm, b->d_pcmf, S, b->nchan, nfr);
    // (the carry in slots 0..2 is not written by k_polyphase, so the two may run in either order)
    // (the detector energies of the carried granule are formed by k_polyphase's first tile of a stream, the carries rolled by
    // k_msscan, flags and block types by one kernel - round 6: three launches less per call, which is what a one-stream call
    // is made of)
    LAUNCH(k_polyphase, g1, dim3(K1_THREADS), q, d_pcm, nsamp, b->d_st, b->d_prm, b->d_gt, b->d_sb, NG, SG, pcmf, b->nchan, b->d_eng, nfr);
    LAUNCH(k_detect, dim3((S + 3) / 4), dim3(256), q, b->d_st, b->d_prm, b->d_eng, b->d_flg, b->debug ? b->d_dbgmetric : nullptr, f.bt, f.btprev, NG, S, nfr);
    // (the form of K4 that goes with the stream-walk kernel: hx_spec.hip, spec_granule)
    if (launch_spec(q, b->slim != 0, b->d_sb, b->d_st, b->d_prm, b->d_gt, f.bt, f.xr, f.etab, f.thr, f.msbase, S, NG, SG, nfr) != 0) return -1;
    // stereo decisions and the pre-echo hand-over (serial per stream) with the carries of the subband buffer and the PCM
    // history (they belong to the front end: k_alloc does not touch them), then the allocator's state-independent start
    // values per granule; the magnitudes replace the spectrum in place, so the tests' tap of it is taken first
    LAUNCH(k_msscan, dim3(S), dim3(64), q, b->d_st, b->d_prm, f.msbase, f.bt, f.msflag, f.msdec, f.thr, f.thrprev, NG, b->d_sb, SG, d_pcm, nsamp, pcmf, b->nchan, nfr);
    LAUNCH(k_prep, dim3((unsigned) (((long long) S * NG + 3) / 4)), dim3(256), q, f.xr, (b->debug && b->d_xrdbg) ? b->d_xrdbg : (float *) nullptr, b->debug ? f.x34 : (float *) nullptr,
           b->sgn[p.sset], f.band, b->d_st, b->d_prm, b->d_gt, f.bt, f.msflag, f.etab, f.thr, f.thrprev, NG, (long long) S * NG, nfr);
    return 0;
}

// a submit's hand-over from the front-end stream to the stream walk's
static int pipe_front_done(hx_batch *b, const Pass &p)
{
    HIPCHK(hipEventRecord(b->ev_front[p.set], p.q));
    HIPCHK(hipStreamWaitEvent(p.qa, b->ev_front[p.set], 0));
    if (b->nsubmit >= 2) HIPCHK(hipStreamWaitEvent(p.qa, b->ev_alloc[p.set], 0));     // the packing of submit n-2 is done with the lines / records of this set
    // A caller that hands consecutive submits the same output buffers gets them one after the other: the previous
    // submit's packing (which writes and reads its `out`) then has to be through before this allocator launch
    // starts putting headers into it.  Alternate two sets of output buffers to have them overlap.
    const hx_batch::PackJob &j = b->pack_job;
    if (j.pending) {
        const Call &jc = j.call, &pc = p.call;
        const unsigned char *o0 = jc.out, *o1 = jc.out + (long long) b->S * jc.out_stride, *n0 = pc.out, *n1 = pc.out + (long long) b->S * pc.out_stride;
        const char *b0 = (const char *) jc.out_bytes, *b1 = b0 + sizeof(int) * (size_t) b->S, *m0 = (const char *) pc.out_bytes, *m1 = m0 + sizeof(int) * (size_t) b->S;
        if ((o0 < n1 && n0 < o1) || (b0 < m1 && m0 < b1)) {
            const int js = j.set;
            if (flush_pack(b, -1) != 0) return -1;
            HIPCHK(hipStreamWaitEvent(p.qa, b->ev_alloc[js], 0));
        }
    }
    return 0;
}

// the stream walk's arguments; with the longest-first order (see hx_batch::lpt), the kernel that sorts the streams
static int fill_alloc_args(hx_batch *b, const Pass &p, AllocArgs &a)
{
    const FrontSet &f = b->front[p.set];
    const WalkSet &w = b->walk[p.set];
    unsigned *const sgn = b->sgn[p.sset];
    const int S = b->S;
    const Call &c = p.call;
    a.st = b->d_st; a.prm = b->d_prm; a.gt = b->d_gt; a.xr = f.xr; a.etab = f.etab; a.thr = f.thr;
    a.msbase = f.msbase; a.bt = f.bt; a.btprev = f.btprev; a.out = c.out; a.out_bytes = c.out_bytes;
    a.dbg = frame_records(b, c, p.set, p.kind); a.out_stride = c.out_stride; a.NG = 2 * p.nframes; a.S = S; a.nfr = c.nfr; a.status = b->d_status; a.prof = b->d_prof;
    a.packet = c.opt.packet; a.packet_stride = c.opt.packet_stride; a.packet_bytes = c.opt.packet_bytes; a.frame_stats = c.opt.frame_stats;
    a.done_counter = b->d_done;
    a.strict_sums = b->strict_sums;
    a.dur = b->d_dur;
    a.order = nullptr;
    a.park_k = 0;
    a.pos0 = 0; a.npos = S; a.fpc = (b->lsf ? 2 : 1) * p.nframes;
    if (several_kinds(b)) {     // the streams partitioned by kind, whatever the batch's size: launch_walk takes the spans
        LAUNCH(k_order_kinds, dim3(1), dim3(1024), p.qa, (const unsigned *) b->d_dur, (const HxStream *) b->d_st, (const HxParams *) b->d_prm, b->d_order, S);
        a.order = b->d_order;
    } else if ((S > b->resident && b->lpt) || (b->lpt == 2 && S > b->ncu) || b->lpt == 3) {
        LAUNCH(k_order, dim3(1), dim3(1024), p.qa, (const unsigned *) b->d_dur, b->d_order, S);
        a.order = b->d_order;
        // parking (hx_alloc3.inc): only when every stream has a slot from the launch's start - beyond the resident set a
        // parked slot would keep a waiting stream out - and from the second call on (the order is the previous call's)
        if (S <= b->resident && b->alloc_launches > 0 && !b->alloc1 && !b->lsf) a.park_k = (b->park_k < S / 8 ? b->park_k : S / 8) | (b->park_pair << 16);
    }
    a.x34 = f.x34; a.sgn = sgn; a.band = f.band; a.msflag = f.msflag; a.msdec = f.msdec; a.thrprev = f.thrprev;
    a.ixq = w.ixq; a.sgn_w = sgn; a.seg = w.seg; a.frm = w.frm; a.slots = w.slots;
    a.pre_len = w.pre_len; a.carry_len = w.carry_len;
    return 0;
}

// the stream walk, between two timing events (hx_batch_alloc_kernel_ms) unless the pass is being recorded
static int launch_walk(hx_batch *b, const Pass &p, const AllocArgs &a)
{
    const hipStream_t qa = p.qa;
    const int S = b->S;
    b->alloc_launches++;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!p.call.recording) {
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipEventRecord(e0, qa));
    }
    // persistent workgroups: as many as the chip holds at once (or one per stream if that is fewer); each walks one stream of
    // the launch order after the other (hx_alloc3.inc)
    // (built into k_alloc_slim, the kernel of batches beyond the resident set; the 256-register kernels keep one workgroup per stream)
    // A batch of several kinds: one launch per kind that has streams, kinds 0 .. 3, each over its span of the order that
    // k_order_kinds made, one after the other on this one stream - the claim and idle counters are the batch's, so two walks
    // never run at once.  The spans come from the host's view of the slots, which is the device's at this point of the stream
    // (an assign moves both, the device in stream order).  Every position of the order is walked by exactly one launch, so a
    // call still adds S to the started-counter, whatever its split.
    int count[4] = {0, 0, 0, 0};
    if (several_kinds(b)) for (int s = 0; s < S; s++) count[b->cls_kind[b->cls_of[s]]]++;
    else count[__builtin_ctz(b->kinds)] = S;
    AllocArgs ak = a;
    for (int kind = 0, pos = 0; kind < 4; pos += count[kind++]) {
        const int n = count[kind];
        if (n == 0) continue;
        ak.pos0 = pos; ak.npos = n;
        const int G = (kind == 0 && b->slim && n > b->resident) ? b->resident : n;
        if (kind == 3) LAUNCH(k_alloc1_lsf, dim3(G), dim3(128), qa, ak);
        else if (kind == 2) LAUNCH(k_alloc1, dim3(G), dim3(128), qa, ak);
        else if (kind == 1) LAUNCH(k_alloc_lsf, dim3(G), dim3(128), qa, ak);
        else if (b->slim) LAUNCH(k_alloc_slim, dim3(G), dim3(128), qa, ak);
        else LAUNCH(k_alloc, dim3(G), dim3(128), qa, ak);
    }
    if (!p.call.recording) {
        HIPCHK(hipEventRecord(e1, qa));
        b->pending.push_back({e0, e1});
    }
    return 0;
}

// Every frame of the call packed at once, between the pending frames' images coming out of the stream state and the
// incomplete ones' going back in.  A plain call (and a host-buffer submit) packs right behind its allocator launch.  A
// device-buffer submit leaves its packing for later: it is enqueued on a stream of its own behind the NEXT submit's
// allocator launch and a gate on it, and so runs - like that submit's successor's front end - in that launch's tail
// instead of between two allocator launches.
static int place_pack(hx_batch *b, const Pass &p)
{
    const hipStream_t qa = p.qa;
    if (p.kind == PASS_SUBMIT_DEVICE) {
        HIPCHK(hipEventRecord(b->ev_k6[p.set], qa));
        if (flush_pack(b, (long long) ((unsigned long long) (b->alloc_launches - 1) * (unsigned long long) b->S)) != 0) return -1;   // the previous submit's
        b->pack_job = {true, p.call, p.nframes, p.set, p.sset};
        return 0;
    }
    if (p.kind != PASS_PLAIN) HIPCHK(hipEventRecord(b->ev_k6[p.set], qa));
    // the previous device-buffer submit's packing went out on the packing stream in pipe_enter: its k_pack_carry writes
    // the carried frame images that this call's k_pack_pre reads
    if (p.flushed_set >= 0) HIPCHK(hipStreamWaitEvent(qa, b->ev_alloc[p.flushed_set], 0));
    if (enqueue_pack(b, p.call, p.nframes, p.set, p.sset, qa) != 0 || enqueue_dense(b, p.call, p.nframes, qa) != 0 || enqueue_crc(b, p.call, p.nframes, qa) != 0 ||
        enqueue_ledger(b, p.call, p.nframes, qa) != 0 || enqueue_file(b, p.call, p.nframes, qa) != 0 ||
        enqueue_recon(b, p.call, p.nframes, p.set, p.sset, p.kind, qa) != 0) return -1;
    if (p.kind != PASS_PLAIN) { HIPCHK(hipEventRecord(b->ev_alloc[p.set], qa)); HIPCHK(hipEventRecord(b->ev_sgn[p.sset], qa)); }
    return 0;
}

// the time between a stream walk's two events (both done), into the batch's sum
static void take_timing(hx_batch *b, const std::pair<hipEvent_t, hipEvent_t> &pr)
{
    float ms = 0;
    if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { b->alloc_ms_sum += ms; b->alloc_calls++; }
    hipEventDestroy(pr.first);
    hipEventDestroy(pr.second);
}
// a caller that never asks for the timings must not accumulate events
static void reap_timings(hx_batch *b)
{
    while (b->pending.size() > 512 && hipEventQuery(b->pending.front().second) == hipSuccess) {
        take_timing(b, b->pending.front());
        b->pending.erase(b->pending.begin());
    }
}

int encode_pass(hx_batch *b, PcmIn in, int nframes, const Call &c, void *stream, PassKind kind)
{
    if (in.image() && rows_reserve(b, in, nframes) != 0) return -1;
    Poison poison{b};
    Pass p = {in, nframes, c, kind, (hipStream_t) stream, (hipStream_t) stream};
    AllocArgs a;
    HIPCHK(hipSetDevice(b->device));
    if (pipe_enter(b, p) != 0 || upload_counts(b, p) != 0 || upload_image(b, p) != 0 || launch_front(b, p) != 0) return -1;
    if (kind != PASS_PLAIN && pipe_front_done(b, p) != 0) return -1;
    if (fill_alloc_args(b, p, a) != 0 || launch_walk(b, p, a) != 0 || place_pack(b, p) != 0) return -1;
    if (!c.recording) reap_timings(b);
    if (kind != PASS_PLAIN) {
        b->nsubmit++;
        b->inflight = true;
    }
    HIPCHK(hipGetLastError());
    b->lastNG = 2 * nframes;
    return poison.ok();
}
int encode_checked(hx_batch *b, PcmIn in, int nframes, const Call &c, void *stream, PassKind kind)
{
    if (check_call(b, in.p, nframes, c.out, c.out_stride, c.out_bytes) != 0 || check_opt(b, c.opt, counts_in_force(b)) != 0 ||
        check_image(b, nframes, in.sample_bytes(), 0) != 0) return -1;
    return encode_pass(b, in, nframes, c, stream, kind);
}

// K-1 alone (include/hmp3_amd.h, hx_batch_debug_pcm_rows): a plain device call's checks, its layout upload and its row
// kernel, and nothing behind them - no stream moves, no output is written; the rows are read with the "pcmrows" tap.
extern "C" int hx_batch_debug_pcm_rows(hx_batch *b, const void *d_pcm, int nframes, int f32, void *stream)
{
    if (!b) { set_err("null batch"); return -1; }
    if (check_poisoned(b) != 0) return -1;
    if (b->nsrc) { set_err("a converting batch has no PCM rows of its own"); return -1; }
    if (!d_pcm) { set_err("null buffer"); return -1; }
    if (nframes <= 0 || nframes > b->maxF) { set_err("nframes out of range (1 .. max_frames)"); return -1; }
    const PcmIn in = pcm_in(b, d_pcm, f32 != 0);
    if (!in.image()) { set_err("hx_batch_debug_pcm_rows needs PCM segments or PCM planes in force"); return -1; }
    if (check_counts(b, nframes, 0) != 0 || check_image(b, nframes, in.sample_bytes(), 0) != 0 || rows_reserve(b, in, nframes) != 0) return -1;
    Poison poison{b};
    Pass p = {in, nframes, Call(), PASS_PLAIN, (hipStream_t) stream, (hipStream_t) stream};
    HIPCHK(hipSetDevice(b->device));
    if (pipe_enter(b, p) != 0 || upload_counts(b, p) != 0 || upload_image(b, p) != 0 || launch_rows(b, p) != 0) return -1;
    HIPCHK(hipGetLastError());
    return poison.ok();
}

extern "C" int hx_batch_encode_s16_device(hx_batch *b, const int16_t *d_pcm, int nframes, unsigned char *d_out,
                                          long long out_stride, int *d_out_bytes, void *stream)
{
    return encode_checked(b, pcm_in(b, d_pcm, false), nframes, call_on(b, d_out, out_stride, d_out_bytes), stream, PASS_PLAIN);
}

extern "C" int hx_batch_encode_f32_device(hx_batch *b, const float *d_pcm, int nframes, unsigned char *d_out,
                                          long long out_stride, int *d_out_bytes, void *stream)
{
    return encode_checked(b, pcm_in(b, d_pcm, true), nframes, call_on(b, d_out, out_stride, d_out_bytes), stream, PASS_PLAIN);
}

// Pipelined form of the device calls.  A submit returns at once like the plain call, but its output
// (d_out, d_out_bytes) is ordered on the caller's stream only by a later hx_batch_wait (or by the next
// plain call / host-buffer call on the batch).  The PCM must be ready on `stream` at the submit, and
// d_pcm must stay unchanged until the submit's front end has run (hx_batch_wait covers that too).
// Consecutive submits overlap: the front end of call n+1 fills the SIMDs that k_alloc of call n
// leaves idle while its slowest streams finish.
extern "C" int hx_batch_submit_s16_device(hx_batch *b, const int16_t *d_pcm, int nframes, unsigned char *d_out,
                                          long long out_stride, int *d_out_bytes, void *stream)
{
    return encode_checked(b, pcm_in(b, d_pcm, false), nframes, call_on(b, d_out, out_stride, d_out_bytes), stream, PASS_SUBMIT_DEVICE);
}

extern "C" int hx_batch_submit_f32_device(hx_batch *b, const float *d_pcm, int nframes, unsigned char *d_out,
                                          long long out_stride, int *d_out_bytes, void *stream)
{
    return encode_checked(b, pcm_in(b, d_pcm, true), nframes, call_on(b, d_out, out_stride, d_out_bytes), stream, PASS_SUBMIT_DEVICE);
}

// share (percent) of the previous allocator launch's resident workgroups that must have started before a submit's front end is released; 0 = no gate
extern "C" void hx_batch_set_gate(hx_batch *b, int percent) { if (b) b->gate_percent = percent < 0 ? 0 : (percent > 100 ? 100 : percent); }

extern "C" int hx_batch_wait(hx_batch *b, void *stream)
{
    if (!b || check_poisoned(b) != 0) return -1;
    if (!b->inflight) return 0;
    Poison poison{b};                   // (the deferred packing may be half enqueued)
    HIPCHK(hipSetDevice(b->device));
    if (order_behind_submits(b, (hipStream_t) stream) != 0) return -1;
    return poison.ok();
}

// ---- pipelined host-buffer calls ----
// The PCM of call n+1 crosses PCIe while call n is encoded, and the bitstream of call n while call
// n+1 is: two sets of device staging buffers, one stream per copy direction, events in between.
// Truly asynchronous only with page-locked host memory (hx_pinned_alloc); with pageable memory the
// copies fall back to staged, mostly synchronous transfers and the result is still correct.
extern "C" void *hx_pinned_alloc(long long bytes)
{
    void *p = nullptr;
    if (bytes <= 0 || hipHostMalloc(&p, (size_t) bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
extern "C" void hx_pinned_free(void *p) { if (p) hipHostFree(p); }

// img: null, or (hx_batch_submit_*_host_dense) the caller's page-locked image and offsets as the device sees them - the
// image kernels of the call write them, and the rows stay in the staging: out is not used
static int submit_host(hx_batch *b, PcmIn in, int nframes, unsigned char *out, long long out_stride, int *out_bytes, const DenseOut *img = nullptr)
{
    if (check_call(b, in.p, nframes, img ? img->buf : out, out_stride, out_bytes) != 0 || check_opt(b, b->opt, counts_in_force(b)) != 0 ||
        check_image(b, nframes, in.sample_bytes(), 0) != 0) return -1;
    // (under segments: the span of the image its segments cover, as in encode_host; the staging is sized by what goes up)
    in = pcm_in(b, in.p, in.f32);
    long long lo = 0, hi = in.bytes(b->S, nframes, b->nchan);
    if (in.image()) image_span(b, in, nframes, lo, hi);
    if (in.image() && rows_reserve(b, in, nframes) != 0) return -1;
    Poison poison{b};                   // (staging buffers, events and the call counter are touched from here on)
    HIPCHK(hipSetDevice(b->device));
    const long long pbytes = hi - lo, obytes = (long long) b->S * out_stride;
    if (!b->s_h2d) {
        if (new_stream(b, b->s_h2d) || new_stream(b, b->s_d2h) || new_stream(b, b->s_host)) return -1;
        for (int i = 0; i < 2; i++)
            if (new_event(b, b->ev_h2d[i]) || new_event(b, b->ev_d2h[i]) || new_event(b, b->ev_hfront[i]) || dev_alloc(b, b->hs_nb[i], sizeof(int) * b->S)) return -1;
    }
    if (pbytes > b->hs_pcm_cap || obytes > b->hs_out_cap) {     // (re)size the staging: drain first
        if (drain(b) != 0) return -1;
        for (int i = 0; i < 2; i++) {
            if (pbytes > b->hs_pcm_cap && dev_realloc(b, b->hs_pcm[i], pbytes) != 0) return -1;
            if (obytes > b->hs_out_cap && dev_realloc(b, b->hs_out[i], obytes) != 0) return -1;
        }
        if (pbytes > b->hs_pcm_cap) b->hs_pcm_cap = pbytes;
        if (obytes > b->hs_out_cap) b->hs_out_cap = obytes;
    }
    if (img && !b->hs_off[0])
        for (int i = 0; i < 2; i++) if (dev_alloc(b, b->hs_off[i], sizeof(long long) * (b->S + 1)) != 0) return -1;
    const int k = (int) (b->nhost & 1);
    if (b->nhost >= 2) {
        HIPCHK(hipStreamWaitEvent(b->s_h2d, b->ev_hfront[k], 0));   // the front end of call n-2 has read this PCM buffer
        HIPCHK(hipStreamWaitEvent(b->s_host, b->ev_d2h[k], 0));     // the bitstream of call n-2 has left this output buffer
    }
    if (pbytes > 0) HIPCHK(hipMemcpyAsync(b->hs_pcm[k], (const char *) in.p + lo, (size_t) pbytes, hipMemcpyHostToDevice, b->s_h2d));
    HIPCHK(hipEventRecord(b->ev_h2d[k], b->s_h2d));
    HIPCHK(hipStreamWaitEvent(b->s_host, b->ev_h2d[k], 0));
    const int set = (int) (b->nsubmit & 1);
    Call c = call_on(b, b->hs_out[k], out_stride, b->hs_nb[k]);
    if (img) c.opt.dense = DenseOut{img->buf, img->cap, b->hs_off[k], img->off};
    PcmIn up = in;
    up.p = b->hs_pcm[k]; up.shift = lo;
    if (encode_pass(b, up, nframes, c, b->s_host, PASS_SUBMIT_HOST) != 0) return -1;
    HIPCHK(hipEventRecord(b->ev_hfront[k], b->s_front));
    HIPCHK(hipStreamWaitEvent(b->s_d2h, b->ev_alloc[set], 0));
    HIPCHK(hipMemcpyAsync(out_bytes, b->hs_nb[k], sizeof(int) * b->S, hipMemcpyDeviceToHost, b->s_d2h));
    if (!img && rows_to_host(b, out, b->hs_out[k], out_stride, b->s_d2h) != 0) return -1;
    HIPCHK(hipEventRecord(b->ev_d2h[k], b->s_d2h));     // (a dense call: its image kernels, which ev_alloc covers, are done)
    b->nhost++;
    return poison.ok();
}

extern "C" int hx_batch_submit_s16_host(hx_batch *b, const int16_t *pcm, int nframes, unsigned char *out, long long out_stride, int *out_bytes)
{
    return submit_host(b, {pcm, false}, nframes, out, out_stride, out_bytes);
}

extern "C" int hx_batch_submit_f32_host(hx_batch *b, const float *pcm, int nframes, unsigned char *out, long long out_stride, int *out_bytes)
{
    return submit_host(b, {pcm, true}, nframes, out, out_stride, out_bytes);
}

// Pipelined host calls that return the dense image only.  Nothing waits for a byte count: k_dense_gather stores the image and
// k_dense_off the offsets straight into the caller's page-locked memory, which the device reaches over the link (the
// one-stream encoder's packing publishes its results the same way); the rows stay in the staging.  The gather reads the
// offsets from a copy in device memory.
// (Kernel-written host memory against the DMA copy of the rows has not been measured: DESIGN.md section 5.)
// [p, p + bytes) as the current device addresses it, or null: page-locked host memory of ONE allocation or registration
// (first and last byte are host memory and lie as far apart for the device as for the host) that is mapped for the device
static void *pinned_device_ptr(const void *p, long long bytes)
{
    const long long span = bytes > 0 ? bytes - 1 : 0;
    hipPointerAttribute_t a0, a1;
    void *dp = nullptr;
    if (hipPointerGetAttributes(&a0, p) != hipSuccess || hipPointerGetAttributes(&a1, (const char *) p + span) != hipSuccess ||
        hipHostGetDevicePointer(&dp, const_cast<void *>(p), 0) != hipSuccess) {
        (void) hipGetLastError();       // (pageable memory is an invalid value to some runtimes, unregistered memory to others)
        return nullptr;
    }
    if (a0.type != hipMemoryTypeHost || a1.type != hipMemoryTypeHost || !dp) return nullptr;
    if ((const char *) a1.devicePointer - (const char *) a0.devicePointer != span || (const char *) a1.hostPointer - (const char *) a0.hostPointer != span) return nullptr;
    return dp;
}
static int submit_host_dense(hx_batch *b, PcmIn in, int nframes, unsigned char *dense, long long dense_cap, long long *dense_off, int *out_bytes)
{
    if (!b) { set_err("null batch"); return -1; }
    if (!dense || !dense_off || dense_cap < 0) { set_err("null buffer"); return -1; }
    if (hipSetDevice(b->device) != hipSuccess) { set_err("hipSetDevice failed"); return -1; }
    DenseOut img;
    img.buf = (unsigned char *) pinned_device_ptr(dense, dense_cap);
    img.off = (long long *) pinned_device_ptr(dense_off, (long long) sizeof(long long) * (b->S + 1));
    img.cap = dense_cap;
    if (!img.buf || !img.off) { set_err("dense and dense_off must be page-locked host memory (hx_pinned_alloc, or registered with the HIP runtime): the image kernels write them"); return -1; }
    if (((unsigned long long) img.buf & 15) != 0) { set_err("dense must be 16-byte aligned"); return -1; }
    if (((unsigned long long) img.off & 7) != 0) { set_err("dense_off must be 8-byte aligned"); return -1; }
    return submit_host(b, in, nframes, nullptr, hx_batch_out_stride(b, nframes), out_bytes, &img);
}
extern "C" int hx_batch_submit_s16_host_dense(hx_batch *b, const int16_t *pcm, int nframes, unsigned char *dense, long long dense_cap,
                                              long long *dense_off, int *out_bytes)
{
    return submit_host_dense(b, {pcm, false}, nframes, dense, dense_cap, dense_off, out_bytes);
}
extern "C" int hx_batch_submit_f32_host_dense(hx_batch *b, const float *pcm, int nframes, unsigned char *dense, long long dense_cap,
                                              long long *dense_off, int *out_bytes)
{
    return submit_host_dense(b, {pcm, true}, nframes, dense, dense_cap, dense_off, out_bytes);
}

// block until the outputs of every submitted host call are in host memory
extern "C" int hx_batch_wait_host(hx_batch *b)
{
    if (!b || check_poisoned(b) != 0) return -1;
    if (hipSetDevice(b->device) != hipSuccess || (b->s_d2h && (hipStreamSynchronize(b->s_front) != hipSuccess || hipStreamSynchronize(b->s_d2h) != hipSuccess))) {
        set_err("HIP error while waiting for the host-buffer calls");
        b->poisoned = true;
        return -1;
    }
    return 0;
}

extern "C" float hx_batch_alloc_kernel_ms(hx_batch *b, int *ncalls)
{
    hipSetDevice(b->device);
    for (auto &pr : b->pending) {
        hipEventSynchronize(pr.second);
        take_timing(b, pr);
    }
    b->pending.clear();
    float mean = b->alloc_calls ? (float) (b->alloc_ms_sum / b->alloc_calls) : 0.0f;
    if (ncalls) *ncalls = b->alloc_calls;
    b->alloc_ms_sum = 0;
    b->alloc_calls = 0;
    return mean;
}

// the host-buffer PCM calls (host_call; the staging is not waited for before the upload: these calls end drained).
// With `stats` also the per-frame counters (see hx_batch_frame_stats_buffer); with hd the dense image instead of the rows.
// files (encode_host_files): no host outputs at all, see host_call.
int encode_host(hx_batch *b, PcmIn in, int nframes, unsigned char *out, long long out_stride, int *out_bytes, int *stats, const HostDense *hd,
                unsigned short *crc, bool files, float *recon)
{
    if (check_call(b, in.p, nframes, hd ? hd->dense : out, out_stride, out_bytes, !files) != 0) return -1;
    if (hd && (!hd->off || hd->cap < 0)) { set_err("null buffer"); return -1; }
    if (check_image(b, nframes, in.sample_bytes(), 0) != 0) return -1;
    // under segments or planes one span of the image goes up, from the lowest segment (plane) start to the highest end; rows: all of them
    in = pcm_in(b, in.p, in.f32);
    long long lo = 0, hi = in.bytes(b->S, nframes, b->nchan);
    if (in.image()) image_span(b, in, nframes, lo, hi);
    return host_call(b, (const char *) in.p + lo, hi - lo, false, nframes, out, out_stride, out_bytes, stats, [&](const Call &c) {
        PcmIn up = in;
        up.p = b->d_in; up.shift = lo;
        return encode_pass(b, up, nframes, c, nullptr, PASS_PLAIN);
    }, hd, crc, files, recon);
}

// what every *_host_files call needs of the batch (hx_multi: for all blocks before one starts)
int check_files(const hx_batch *b)
{
    if (!b) { set_err("null batch"); return -1; }
    if (!b->d_ledger) { set_err("a *_host_files call needs a file ledger (hx_batch_ledger_begin)"); return -1; }
    if (!b->files.img) { set_err("a *_host_files call needs file images (hx_batch_file_images)"); return -1; }
    return 0;
}
// The host calls that bring nothing down but the status: rows, byte counts, counters and CRCs stay in the batch's staging,
// from which the ledger and the file images advance.
int encode_host_files(hx_batch *b, PcmIn in, int nframes)
{
    if (check_files(b) != 0) return -1;
    return encode_host(b, in, nframes, nullptr, hx_batch_out_stride(b, nframes), nullptr, nullptr, nullptr, nullptr, true);
}
extern "C" int hx_batch_encode_s16_host_files(hx_batch *b, const int16_t *pcm, int nframes) { return encode_host_files(b, {pcm, false}, nframes); }
extern "C" int hx_batch_encode_f32_host_files(hx_batch *b, const float *pcm, int nframes) { return encode_host_files(b, {pcm, true}, nframes); }

extern "C" int hx_batch_encode_s16_host(hx_batch *b, const int16_t *pcm, int nframes, unsigned char *out,
                                        long long out_stride, int *out_bytes)
{
    return encode_host(b, {pcm, false}, nframes, out, out_stride, out_bytes, nullptr);
}

extern "C" int hx_batch_encode_f32_host_stats(hx_batch *b, const float *pcm, int nframes, unsigned char *out,
                                              long long out_stride, int *out_bytes, int *stats)
{
    if (!stats) { set_err("null buffer"); return -1; }
    return encode_host(b, {pcm, true}, nframes, out, out_stride, out_bytes, stats);
}

extern "C" int hx_batch_encode_f32_host_crc(hx_batch *b, const float *pcm, int nframes, unsigned char *out,
                                            long long out_stride, int *out_bytes, int *stats, unsigned short *crc)
{
    if (!stats || !crc) { set_err("null buffer"); return -1; }
    return encode_host(b, {pcm, true}, nframes, out, out_stride, out_bytes, stats, nullptr, crc);
}

// ... with the decoded PCM of the call (hx_batch_recon_buffer) in host memory, through staging: a buffer set on the batch is not written
extern "C" int hx_batch_encode_f32_host_recon(hx_batch *b, const float *pcm, int nframes, unsigned char *out,
                                              long long out_stride, int *out_bytes, float *recon)
{
    if (!recon) { set_err("null buffer"); return -1; }
    if (recon_refused(b) != 0) return -1;
    return encode_host(b, {pcm, true}, nframes, out, out_stride, out_bytes, nullptr, nullptr, nullptr, false, recon);
}

extern "C" int hx_batch_encode_f32_host(hx_batch *b, const float *pcm, int nframes, unsigned char *out,
                                        long long out_stride, int *out_bytes)
{
    return encode_host(b, {pcm, true}, nframes, out, out_stride, out_bytes, nullptr);
}

// The synchronous host calls that return the dense image: rows, image and offsets in device staging, and only the byte
// counts, the offsets and the image's used part cross the link.  (An image that does not fit dense_cap: the segments that
// fit in whole are a prefix of the streams, and that prefix is what is copied.)
static int encode_host_dense(hx_batch *b, PcmIn in, int nframes, unsigned char *dense, long long dense_cap, long long *dense_off, int *out_bytes)
{
    const HostDense hd = {dense, dense_cap, dense_off, hx_batch_dense_bound(b, nframes)};
    return encode_host(b, in, nframes, nullptr, hx_batch_out_stride(b, nframes), out_bytes, nullptr, &hd);
}
extern "C" int hx_batch_encode_s16_host_dense(hx_batch *b, const int16_t *pcm, int nframes, unsigned char *dense, long long dense_cap,
                                              long long *dense_off, int *out_bytes)
{
    return encode_host_dense(b, {pcm, false}, nframes, dense, dense_cap, dense_off, out_bytes);
}
extern "C" int hx_batch_encode_f32_host_dense(hx_batch *b, const float *pcm, int nframes, unsigned char *dense, long long dense_cap,
                                              long long *dense_off, int *out_bytes)
{
    return encode_host_dense(b, {pcm, true}, nframes, dense, dense_cap, dense_off, out_bytes);
}

extern "C" int hx_batch_status(hx_batch *b)
{
    int v = -1;
    if (!b) return -1;
    if (b->poisoned) return -1;
    if (drain(b) != 0) return -1;       // (the last device-buffer submit's packing: it writes that submit's output buffers)
    // (a gate that gave up waiting costs overlap, not correctness: it is counted in hx_batch_gate_timeouts, not here)
    if (hipMemcpy(&v, b->d_status, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v;
}

// which build of the stream walk the batch runs: 0 = k_alloc (or the MPEG-2 / first-generation kernels), 1 = k_alloc_slim;
// streams resident at once on the device
extern "C" int hx_batch_k6_variant(const hx_batch *b) { return b ? b->slim : -1; }
extern "C" int hx_batch_resident_streams(const hx_batch *b) { return b ? b->resident : -1; }

// submits whose front end started late because its gate gave up waiting (see hx_batch_set_gate); synchronises
extern "C" int hx_batch_gate_timeouts(hx_batch *b)
{
    int v[HX_CNT_GATE_TIMEOUTS + 1] = {};
    if (!b) return -1;
    if (drain(b) != 0) return -1;
    if (hipMemcpy(v, b->d_done, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v[HX_CNT_GATE_TIMEOUTS];
}

extern "C" HX_INT_PAIR hx_batch_frames_bytes(hx_batch *b, int i)
{
    HX_INT_PAIR r = {0, 0};
    if (!b || i < 0 || i >= b->S) return r;
    (void) drain(b);
    unsigned v[2];
    hipMemcpy(&v[0], (char *) (b->d_st + i) + offsetof(HxStream, tot_frames_out), 4, hipMemcpyDeviceToHost);
    hipMemcpy(&v[1], (char *) (b->d_st + i) + offsetof(HxStream, tot_bytes_out), 4, hipMemcpyDeviceToHost);
    r.a = (int) v[0]; r.b = (int) v[1];
    return r;
}

// For tests: ix^(4/3) as the device's pow() returns it, the expression of pow43_beyond (hx_alloc.hip) and of the short-block
// noise measurement (hx_alloc_short.inc), for ix = first .. first + n - 1.  The only kernel of this unit.
__global__ void k_debug_pow43(double *out, int first, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pow((double) (first + i), (4.0 / 3.0));
}

static long long debug_pow43(void *dst, long long cap)
{
    const long long n = cap / (long long) sizeof(double);
    if (n <= 0 || n > (1LL << 24)) return -1;
    double *d = nullptr;
    if (hipMalloc(&d, sizeof(double) * n) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_debug_pow43, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, d, HX_POW43_N, (int) n);
    const hipError_t e = hipMemcpy(dst, d, sizeof(double) * n, hipMemcpyDeviceToHost);
    (void) hipFree(d);
    return e == hipSuccess ? (long long) sizeof(double) * n : -1;
}

extern "C" long long hx_batch_debug_read(hx_batch *b, const char *name, void *dst, long long cap)
{
    if (!b || !name || !dst) return -1;
    (void) drain(b);
    if (!strcmp(name, "pow43_beyond")) return debug_pow43(dst, cap);      // double [cap / 8]: the device's pow(ix, 4/3), ix = HX_POW43_N + i
    const long long S = b->S, NG = b->lastNG;
    const FrontSet &f = b->front[0];
    const WalkSet &w = b->walk[0];
    const void *src = nullptr;
    long long n = 0;
    std::string k(name);
    if (k == "sb") { src = b->d_sb; n = sizeof(float) * S * 2 * (2LL * b->maxF + 3) * 576; }
    else if (k == "xr") { src = f.xr; n = sizeof(float) * S * NG * 1152; }       // the spectrum
    else if (k == "xmag") { src = b->d_xrdbg; n = sizeof(float) * S * NG * 1152; }  // the magnitudes k_prep works on (written in debug mode only)
    else if (k == "x34") { src = f.x34; n = sizeof(float) * S * NG * 1152; }
    else if (k == "band") { src = f.band; n = sizeof(HxBandPrep) * S * NG; }
    else if (k == "msflag") { src = f.msflag; n = S * NG; }
    else if (k == "ixq") { src = w.ixq; n = sizeof(short) * S * NG * 1152; }
    else if (k == "sgn") { src = b->sgn[0]; n = (long long) sizeof(unsigned) * S * NG * 2 * HX_SGN_WORDS; }      // one bit per line, HX_SGN_WORDS words per (granule, channel)
    else if (k == "seg") { src = w.seg; n = sizeof(HxSegOut) * S * NG * 2; }
    else if (k == "frm") { src = w.frm; n = sizeof(HxFrameOut) * S * NG; }
    else if (k == "etab") { src = f.etab; n = sizeof(float) * S * NG * 128; }
    else if (k == "thr") { src = f.thr; n = sizeof(float) * S * NG * 128; }
    else if (k == "thrprev") { src = f.thrprev; n = sizeof(float) * S * 128; }      // the pre-echo memory the last call started with (rows of streams that took no frame: not written)
    else if (k == "msbase") { src = f.msbase; n = sizeof(int) * S * NG; }
    else if (k == "place") { src = b->d_dur + S; n = sizeof(unsigned) * S; }       // per WORKGROUP of the last allocator launch (launch order): XCC id << 16 | HW_ID[15:0] (CU [11:8], SH [12], SE [15:13])
    else if (k == "dur") { src = b->d_dur; n = sizeof(unsigned) * S; }              // the last allocator launch's per-stream durations, 100 MHz ticks
    else if (k == "big_sweeps") { src = b->d_done + HX_CNT_BIG_SWEEPS; n = sizeof(int); }        // gain-search line passes that took the double x^(4/3) table
    else if (k == "strict_sums") { src = b->d_done + HX_CNT_STRICT_SUMS; n = sizeof(int); }       // certified band sums that fell back to the strict line-order sum
    else if (k == "lucky") { src = b->d_done + HX_CNT_LUCKY; n = 3 * sizeof(int); }       // big_lucky_noise: granules measured, passes, granules with a pass of more than six candidates (k_alloc_slim does not count)
    else if (k == "lucky_rounds") { src = b->d_done + HX_CNT_LUCKY_ROUNDS; n = 3 * sizeof(int); }       // big_lucky_noise's work lists: entries summed, rounds beyond a wave's first, the longest list of a pass
    else if (k == "bt") { src = f.bt; n = S * NG; }
    else if (k == "eng") { src = b->d_eng; n = sizeof(int) * S * 2 * NG * 9; }
    else if (k == "dbg" && b->d_dbg) { src = b->d_dbg; n = sizeof(HxFrameDebug) * S * (NG / 2); }
    else if (k == "prof" && b->d_prof) { src = b->d_prof; n = sizeof(unsigned long long) * S * HX_PROF_WORDS; }
    else if (k == "state") { src = b->d_st; n = sizeof(HxStream) * S; }
    else if (k == "srcpcm" && b->d_src_pcm) { src = b->d_src_pcm; n = sizeof(float) * S * b->src_lastF * 1152 * b->nchan; }   // the converted PCM of the last call
    else if (k == "pcmrows" && b->d_rows) { src = b->d_rows; n = b->rows_bytes; }      // the row buffer as the last call under PCM segments or planes left it (its stride: that call's nframes and sample type)
    else if (k == "attack" && b->d_dbgmetric) { src = b->d_dbgmetric; n = sizeof(int) * S * NG * 4; }      // [S][NG][4]: the attack metric of channel 0 / 1 for short_flag_prev = 0, then for 1
    if (!src) return -1;
    if (n > cap) n = cap;
    hipMemcpy(dst, src, (size_t) n, hipMemcpyDeviceToHost);
    return n;
}

// For tests: the device math of the kernels on arguments of the caller's (include/hmp3_amd.h).  k_debug_math lives in the
// k_alloc1 unit (hx_alloc1.inc), where every function it calls is compiled with the allocator kernels' flags; the tables are
// this batch's (HxGlobalTabs, the HxParams of its first class).
static const struct { const char *name; int fn, nin; } debug_math_fns[] = {
    {"logf", HX_DM_LOGF, 1}, {"log10f", HX_DM_LOG10F, 1}, {"a1_mask_db", HX_DM_A1_MASK_DB, 2}, {"a1_gz", HX_DM_A1_GZ, 1},
    {"dblog", HX_DM_DBLOG, 1}, {"dual_g", HX_DM_DUAL_G, 1}, {"is_scale", HX_DM_IS_SCALE, 3}, {"is_scale_lsf", HX_DM_IS_SCALE_LSF, 3},
    {"div", HX_DM_DIV, 2}, {"mblog", HX_DM_MBLOG, 1}, {"mblog16", HX_DM_MBLOG16, 1}, {"mbexp", HX_DM_MBEXP, 1},
    {"pow34", HX_DM_POW34, 1}, {"round", HX_DM_ROUND, 1}};
static_assert(sizeof(debug_math_fns) / sizeof(debug_math_fns[0]) == HX_DM_COUNT, "one name per HxDebugMath value");

extern "C" int hx_batch_debug_math(hx_batch *b, const char *name, const void *in, long long n, void *out)
{
    if (!b || !name || !in || !out) { set_err("null argument"); return -1; }
    int fn = -1, nin = 0;
    for (const auto &f : debug_math_fns) if (!strcmp(name, f.name)) { fn = f.fn; nin = f.nin; }
    if (fn < 0) { set_err("hx_batch_debug_math: no function named %s", name); return -1; }
    if (n <= 0 || n > HX_DEBUG_MATH_MAX) { set_err("hx_batch_debug_math takes 1 .. 2^25 arguments per call"); return -1; }
    if (drain(b) != 0) return -1;
    struct Dev {
        unsigned *in = nullptr, *out = nullptr;
        ~Dev() { (void) hipFree(in); (void) hipFree(out); }
    } d;
    const size_t bytes = sizeof(unsigned) * (size_t) n;
    HIPCHK(hipMalloc(&d.in, bytes * nin));
    HIPCHK(hipMalloc(&d.out, bytes));
    HIPCHK(hipMemcpy(d.in, in, bytes * nin, hipMemcpyHostToDevice));
    LAUNCH(k_debug_math, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, fn, d.in, n, d.out, b->d_gt, b->d_prm);
    HIPCHK(hipMemcpy(out, d.out, bytes, hipMemcpyDeviceToHost));
    return 0;
}


// ---- hx_debug_pack: k_pack on records of the caller's (tests only; include/hmp3_amd.h) ----
// What the packer reads of a call - segment records, lines, signs, frame records, slot lists - comes from the caller instead
// of the stream walk; the kernel and its launch are the batch's (launch_pack).  Every record is checked on the host first:
// one the stream walk cannot emit is refused with a message before anything is launched, so nothing the kernel indexes with
// a record's value - a code table, the 640-word bit buffer, the slot list, a row, the packet buffer - can leave its bounds.

// HxFrameOut::near: copies of the frame's first four slots, as the stream walk's helper wave gathers them from its ring
// (hx_alloc3.inc, outbox_gather); entries past the list are never used by the packer and stay zero here
static void frame_near(HxFrameOut &fo, const HxSlot *sl, int nslots)
{
    for (int k = 0; k < 4; k++) {
        const int j = fo.first_slot + k;
        fo.near[k] = (j >= 0 && j < nslots) ? sl[j] : HxSlot{0, 0};
    }
}

static int pack_refuse(long long s, long long f, int w, const char *what)
{
    char msg[256];
    if (w >= 0) snprintf(msg, sizeof msg, "stream %lld frame position %lld segment %d: %s", s, f, w, what);
    else snprintf(msg, sizeof msg, "stream %lld frame position %lld: %s", s, f, what);
    set_err("%s", msg);
    return -1;
}

static int check_pack_records(const std::vector<HxParams> &prm, const HxGlobalTabs &gt, const int *cls, int S, int NG, int fps, const int *nfr,
                              const HxSegOut *seg, const short *ixq, const HxFrameOut *frm, const HxSlot *slots, long long out_stride,
                              const unsigned char *packet, long long packet_bytes)
{
    const int nslots = fps + HX_SLOTS_EXTRA;
    for (long long s = 0; s < S; s++) {
        const HxParams &p = prm[cls[s]];
        const int lsf = !p.h_id, nchan = p.nchan, hdr = 4 + p.side_bytes;
        const int nf = (lsf ? 2 : 1) * (nfr ? nfr[s] : NG / 2);
        const HxSlot *sl = slots + s * nslots;
        for (int f = 0; f < nf; f++) {
            const HxFrameOut &fo = frm[s * fps + f];
            int pos = 0;
            for (int w = 0; w < (lsf ? 2 : 4); w++) {
                const int g = lsf ? f : 2 * f + (w >> 1), ch = w & 1;
                if (ch >= nchan) continue;
                const long long unit = (s * NG + g) * 2 + ch;
                const HxSegOut &so = seg[unit];
                const short *ix = ixq + unit * 576;
                if (so.start_bit != pos) return pack_refuse(s, f, w, "start_bit is not the end of the segment before it");
                int bits = 0;
                for (int j = 0; j < 40; j++) {
                    const int fld = so.sf[j], len = (fld >> 8) & 15, v = fld & 255;
                    if (!fld) continue;
                    if (fld & 0x7000) return pack_refuse(s, f, w, "a scalefactor field has bits 12 .. 14 set");
                    if (len > 5) return pack_refuse(s, f, w, "a scalefactor field is longer than 5 bits");
                    if ((fld & 0x8000) ? v < 128 : (v >> len) != 0) return pack_refuse(s, f, w, "a scalefactor field's value does not fit its length or its sign flag");
                    bits += len;
                }
                if (so.not_null != 0 && so.not_null != 1) return pack_refuse(s, f, w, "not_null is neither 0 nor 1");
                if (so.not_null) {
                    const int n0 = so.nreg01 & 0xFFFF, n1 = so.nreg01 >> 16, n2 = so.nreg2_quads & 0xFFFF, nq = so.nreg2_quads >> 16, npairs = n0 + n1 + n2;
                    const int t3[3] = {(int) (so.tabs & 255), (int) ((so.tabs >> 8) & 255), (int) ((so.tabs >> 16) & 255)}, c1 = (int) (so.tabs >> 24);
                    if (npairs > 288 || nq > 144 || 2 * npairs + 4 * nq > 576) return pack_refuse(s, f, w, "more than 576 lines in pairs and quads");
                    if (c1 > 1) return pack_refuse(s, f, w, "count1 table above 1");
                    for (int r = 0; r < 3; r++)
                        if (t3[r] > 31 || t3[r] == 4 || t3[r] == 14) return pack_refuse(s, f, w, "a Huffman table the format does not have");
                    for (int pi = 0; pi < npairs; pi++) {
                        const int t = t3[pi < n0 ? 0 : (pi < n0 + n1 ? 1 : 2)], x = ix[2 * pi], y = ix[2 * pi + 1];
                        const int dim = t >= 16 ? 16 : gt.huff_dim[t], lin = t >= 16 ? gt.huff_lin[t] : 0, top = t >= 16 ? 15 + (1 << lin) - 1 : dim - 1;
                        if (x < 0 || y < 0 || x > std::max(top, 0) || y > std::max(top, 0)) return pack_refuse(s, f, w, "a value above its table's range");
                        if (!t) continue;
                        bits += gt.huff_len[gt.huff_off[t] + std::min(x, 15) * dim + std::min(y, 15)] + (x >= 15 ? lin : 0) + (y >= 15 ? lin : 0) + (x != 0) + (y != 0);
                    }
                    for (int q = 0; q < nq; q++) {
                        const short *v = ix + 2 * npairs + 4 * q;
                        for (int k = 0; k < 4; k++) if (v[k] != 0 && v[k] != 1) return pack_refuse(s, f, w, "a count1 value that is neither 0 nor 1");
                        bits += (c1 ? 4 : gt.quada_len[(v[0] << 3) + (v[1] << 2) + (v[2] << 1) + v[3]]) + v[0] + v[1] + v[2] + v[3];
                    }
                }
                if (bits > 4095) return pack_refuse(s, f, w, "longer than 4095 bits");
                pos += bits;
            }
            if (pos > 640 * 32) return pack_refuse(s, f, -1, "main data beyond the packer's bit buffer");
            if (fo.raw_bytes != (pos + 7) >> 3) return pack_refuse(s, f, -1, "raw_bytes is not the segments' bits rounded up to bytes");
            if (fo.bytes < fo.raw_bytes) return pack_refuse(s, f, -1, "bytes below raw_bytes");
            if (fo.first_slot < 0 || fo.first_slot >= nslots || fo.main_bytes < 0) return pack_refuse(s, f, -1, "first_slot or main_bytes out of range");
            long long q = fo.main_bytes;
            int left = fo.bytes, k = fo.first_slot;
            while (left > 0) {
                if (k >= nslots) return pack_refuse(s, f, -1, "the slots from first_slot on hold less than the frame's bytes");
                if (sl[k].mf < 0) return pack_refuse(s, f, -1, "a slot of negative capacity");
                if (q >= sl[k].mf) { q -= sl[k].mf; k++; continue; }
                if (sl[k].off < 0 || (long long) sl[k].off + hdr + sl[k].mf > out_stride) return pack_refuse(s, f, -1, "a slot outside the row");
                const int take = (int) std::min<long long>(left, sl[k].mf - q);
                left -= take; q += take;
            }
            if (fo.packet_off >= 0 && (!packet || fo.packet_off + fo.raw_bytes > packet_bytes)) return pack_refuse(s, f, -1, "packet_off outside the packet buffer");
        }
    }
    return 0;
}

extern "C" int hx_debug_pack(int device, const HX_E_CONTROL *ec, int ncls, const int *cls, int S, int NG, int fps, const int *nfr,
                             const void *seg, const short *ixq, const unsigned *sgn, const void *frm, const void *slots,
                             unsigned char *rows, long long out_stride, unsigned char *packet, long long packet_bytes, int *status)
{
    if (!ec || !cls || !seg || !ixq || !sgn || !frm || !slots || !rows || !status) { set_err("null buffer"); return -1; }
    if (ncls <= 0 || S <= 0 || NG <= 0 || (NG & 1) || (long long) S * NG > (1LL << 20) || out_stride <= 0 || packet_bytes < 0) { set_err("bad arguments"); return -1; }
    // the classes, resolved the way batch_create resolves a menu's entries
    std::vector<HxParams> prm(ncls);
    bool any_lsf = false;
    for (int k = 0; k < ncls; k++) {
        if (!hx_resolve((const HxControl *) (ec + k), &prm[k])) { set_err("configuration rejected"); return -1; }
        any_lsf = any_lsf || !prm[k].h_id;
    }
    for (int s = 0; s < S; s++) if (cls[s] < 0 || cls[s] >= ncls) { set_err("a stream's class is out of range"); return -1; }
    // frame positions per stream (AllocArgs::fpc)
    if (fps != (any_lsf ? NG : NG / 2)) { set_err("the frame stride is NG with an MPEG-2 class in play, else NG / 2"); return -1; }
    if (check_counts_arg(nfr, S, NG / 2, 0) != 0) return -1;
    std::vector<HxGlobalTabs> gt_host(1);
    hx_global_tabs(&gt_host[0]);
    const int nslots = fps + HX_SLOTS_EXTRA;
    if (check_pack_records(prm, gt_host[0], cls, S, NG, fps, nfr, (const HxSegOut *) seg, ixq, (const HxFrameOut *) frm, (const HxSlot *) slots,
                           out_stride, packet, packet_bytes) != 0) return -1;
    std::vector<HxFrameOut> fo((const HxFrameOut *) frm, (const HxFrameOut *) frm + (size_t) S * fps);
    for (long long i = 0; i < (long long) S * fps; i++) frame_near(fo[i], (const HxSlot *) slots + (i / fps) * nslots, nslots);
    std::vector<HxStream> st(S);
    for (int s = 0; s < S; s++) hx_stream_reset(&prm[cls[s]], cls[s], &st[s]);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_err("no HIP device available: the encoder has no CPU fallback"); return -1; }
    if (device < 0 || device >= ndev) { set_err("device index out of range"); return -1; }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { set_err("device is %s: this library runs on gfx950 (MI355X) only", prop.gcnArchName); return -1; }
    HIPCHK(hipSetDevice(device));
    // device copies: everything is released on every way out
    struct Dev {
        std::vector<void *> mem;
        ~Dev() { for (void *p : mem) (void) hipFree(p); }
        void *up(const void *src, size_t bytes)
        {
            void *q = nullptr;
            if (hipMalloc(&q, bytes ? bytes : 16) != hipSuccess) return nullptr;
            mem.push_back(q);
            if (src && bytes && hipMemcpy(q, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
            return q;
        }
    } dev;
    const size_t units = (size_t) S * NG * 2;
    const int zero = 0;
    void *d_st = dev.up(st.data(), sizeof(HxStream) * S), *d_prm = dev.up(prm.data(), sizeof(HxParams) * ncls), *d_gt = dev.up(&gt_host[0], sizeof(HxGlobalTabs));
    void *d_ixq = dev.up(ixq, sizeof(short) * 576 * units), *d_sgn = dev.up(sgn, sizeof(unsigned) * HX_SGN_WORDS * units), *d_seg = dev.up(seg, sizeof(HxSegOut) * units);
    void *d_frm = dev.up(fo.data(), sizeof(HxFrameOut) * fo.size()), *d_slots = dev.up(slots, sizeof(HxSlot) * (size_t) S * nslots);
    void *d_rows = dev.up(rows, (size_t) S * out_stride), *d_packet = packet ? dev.up(packet, (size_t) packet_bytes) : nullptr;
    void *d_status = dev.up(&zero, sizeof(int)), *d_nfr = nfr ? dev.up(nfr, sizeof(int) * S) : nullptr;
    if (!d_st || !d_prm || !d_gt || !d_ixq || !d_sgn || !d_seg || !d_frm || !d_slots || !d_rows || (packet && !d_packet) || !d_status || (nfr && !d_nfr)) {
        set_err("hipMalloc or upload failed");
        return -1;
    }
    if (launch_pack(nullptr, (const HxStream *) d_st, (const HxParams *) d_prm, (const HxGlobalTabs *) d_gt, (const short *) d_ixq, (const unsigned *) d_sgn,
                    (const HxSegOut *) d_seg, (const HxFrameOut *) d_frm, (const HxSlot *) d_slots, (unsigned char *) d_rows, out_stride,
                    (unsigned char *) d_packet, (int *) d_status, fps, NG, (long long) S * fps, (const int *) d_nfr) != 0) return -1;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(rows, d_rows, (size_t) S * out_stride, hipMemcpyDeviceToHost));
    if (packet && packet_bytes) HIPCHK(hipMemcpy(packet, d_packet, (size_t) packet_bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(status, d_status, sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}


// ---- hx_debug_recon: the decoded-PCM kernels on records of the caller's (tests only; include/hmp3_amd.h) ----
// What the three kernels read of a call - lines, signs, segment records, frame records, the carried state - comes from the
// caller instead of the stream walk; the kernels and their launch are the batch's (launch_recon), the tables hx_recon_tabs'.
// Every record a kernel will read is checked on the host first: one the kind-0 stream walk cannot hand over is refused with
// a message before anything is launched.  What no kernel reads - records behind a stream's count, a mono stream's second
// channel, lines from the coded range on - is not looked at.

static int recon_refuse(long long s, int g, int ch, const char *what)
{
    char msg[256];
    if (g < 0) snprintf(msg, sizeof msg, "hx_debug_recon: stream %lld: %s", s, what);
    else if (ch < 0) snprintf(msg, sizeof msg, "hx_debug_recon: stream %lld granule %d: %s", s, g, what);
    else snprintf(msg, sizeof msg, "hx_debug_recon: stream %lld granule %d channel %d: %s", s, g, ch, what);
    set_err("%s", msg);
    return -1;
}

static int check_recon_records(const std::vector<HxParams> &prm, const int *cls, int S, int NG, const int *nfr, const short *ixq,
                               const HxSegOut *seg, const HxFrameDebug *rec, const float *state, long long row)
{
    // (previous, this) block types a stream can have: long 0 -> 0 / 1, start 1 -> 2, short 2 -> 2 / 3, stop 3 -> 0 / 1
    static const unsigned char legal[4][4] = {{1, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 1, 1}, {1, 1, 0, 0}};
    for (long long s = 0; s < S; s++) {
        const int nchan = prm[cls[s]].nchan, nf = nfr ? nfr[s] : NG / 2;
        if (nf == 0) continue;
        if ((long long) nf * 1152 * nchan > row) return recon_refuse(s, -1, -1, "row is shorter than the stream's blocks");
        const float *st = state + s * HX_RECON_STATE_FLOATS;
        for (int ch = 0; ch < nchan; ch++) {
            for (int i = 0; i < 576; i++) if (!std::isfinite(st[ch * 576 + i])) return recon_refuse(s, -1, -1, "state: a tail that is not finite");
            for (int i = 0; i < HX_RECON_HIST_SLOTS * 32; i++)
                if (!std::isfinite(st[HX_RECON_TAIL_FLOATS + ch * HX_RECON_HIST_SLOTS * 32 + i])) return recon_refuse(s, -1, -1, "state: a carried slot that is not finite");
        }
        int bt_prev = -1;
        for (int g = 0; g < 2 * nf; g++) {
            const HxFrameDebug &fr = rec[s * (NG / 2) + (g >> 1)];
            if (fr.ms != 0 && fr.ms != 1) return recon_refuse(s, g, -1, "ms is neither 0 nor 1");
            const int bt = fr.gr[g & 1][0].block_type;
            for (int ch = 0; ch < nchan; ch++) {
                const HxGr &q = fr.gr[g & 1][ch];
                const long long unit = (s * NG + g) * 2 + ch;
                if (q.block_type < 0 || q.block_type > 3) return recon_refuse(s, g, ch, "block_type outside 0 .. 3");
                if (q.block_type != bt) return recon_refuse(s, g, ch, "block_type differs between the channels");
                if (q.mixed_block_flag != 0) return recon_refuse(s, g, ch, "mixed_block_flag set");
                if (q.global_gain < 0 || q.global_gain > 255) return recon_refuse(s, g, ch, "global_gain outside 0 .. 255");
                for (int w = 0; w < 3; w++) if (q.subblock_gain[w] < 0 || q.subblock_gain[w] > 7) return recon_refuse(s, g, ch, "subblock_gain outside 0 .. 7");
                if (q.big_values < 0 || q.big_values > 288) return recon_refuse(s, g, ch, "big_values outside 0 .. 288");
                if (q.aux_nquads < 0) return recon_refuse(s, g, ch, "aux_nquads negative");
                if (bt == 2) {
                    for (int j = 0; j < 36; j++) {
                        const int fld = seg[unit].sf[j], v = fld & 255;
                        if (fld & 0x8000) return recon_refuse(s, g, ch, "a negative short scalefactor field");
                        if (v > (j < 18 ? 15 : 7)) return recon_refuse(s, g, ch, "a short scalefactor field above 15 (bands 0 .. 5) or 7 (bands 6 .. 11)");
                    }
                } else {
                    for (int b = 0; b < 22; b++) {
                        const int v = fr.sf[g & 1][ch][b];
                        if (v < 0 || v > (b < 11 ? 15 : b < 21 ? 7 : 0)) return recon_refuse(s, g, ch, "sf: a long scalefactor outside 0 .. 15 (bands 0 .. 10), 0 .. 7 (bands 11 .. 20) or 0 (band 21)");
                    }
                }
                const int ncoded = q.aux_not_null ? std::min(576, 2 * q.big_values + 4 * q.aux_nquads) : 0;
                for (int j = 0; j < ncoded; j++) {
                    const int mag = ixq[unit * 576 + j];
                    if (mag < 0 || mag > 8206) return recon_refuse(s, g, ch, "ixq: a magnitude outside 0 .. 8206 within the coded range");
                }
            }
            if (bt_prev >= 0 && !legal[bt_prev][bt]) return recon_refuse(s, g, -1, "block_type cannot follow the granule before it");
            bt_prev = bt;
        }
    }
    return 0;
}

extern "C" int hx_debug_recon(int device, const HX_E_CONTROL *ec, int ncls, const int *cls, int S, int NG, const int *nfr,
                              const short *ixq, const unsigned *sgn, const void *seg, const void *rec, float *state, float *hyb,
                              float *out, long long row)
{
    if (!ec || !cls || !ixq || !sgn || !seg || !rec || !state || !hyb || !out) { set_err("null buffer"); return -1; }
    if (ncls <= 0 || S <= 0 || NG <= 0 || (NG & 1) || (long long) S * NG > (1LL << 16) || row <= 0 || row > (1LL << 26)) { set_err("bad arguments"); return -1; }
    std::vector<HxParams> prm(ncls);
    for (int k = 0; k < ncls; k++) {
        if (!hx_resolve((const HxControl *) (ec + k), &prm[k])) { set_err("configuration rejected"); return -1; }
        const HxParams &p = prm[k];
        if (p.alloc1 || !p.h_id) {     // (recon_refused's rule and words)
            char msg[256];
            snprintf(msg, sizeof msg, "decoded PCM covers MPEG-1 streams of the second-generation allocator only: class %d (%d Hz, mode %d%s) is %s",
                     k, p.samprate, p.h_mode, p.is_flag ? ", intensity stereo" : "", p.h_id ? "coded by the first-generation allocator" : "an MPEG-2 rate");
            set_err("%s", msg);
            return -1;
        }
    }
    for (int s = 0; s < S; s++) if (cls[s] < 0 || cls[s] >= ncls) { set_err("a stream's class is out of range"); return -1; }
    if (check_counts_arg(nfr, S, NG / 2, 0) != 0) return -1;
    if (check_recon_records(prm, cls, S, NG, nfr, ixq, (const HxSegOut *) seg, (const HxFrameDebug *) rec, state, row) != 0) return -1;
    std::vector<HxGlobalTabs> gt_host(1);
    std::vector<HxReconTabs> rt_host(1);
    hx_global_tabs(&gt_host[0]);
    hx_recon_tabs(&rt_host[0], &gt_host[0]);
    std::vector<HxStream> st(S);
    for (int s = 0; s < S; s++) hx_stream_reset(&prm[cls[s]], cls[s], &st[s]);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_err("no HIP device available: the encoder has no CPU fallback"); return -1; }
    if (device < 0 || device >= ndev) { set_err("device index out of range"); return -1; }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { set_err("device is %s: this library runs on gfx950 (MI355X) only", prop.gcnArchName); return -1; }
    HIPCHK(hipSetDevice(device));
    struct Dev {        // device copies: everything is released on every way out
        std::vector<void *> mem;
        ~Dev() { for (void *p : mem) (void) hipFree(p); }
        void *up(const void *src, size_t bytes)
        {
            void *q = nullptr;
            if (hipMalloc(&q, bytes) != hipSuccess) return nullptr;
            mem.push_back(q);
            if ((src ? hipMemcpy(q, src, bytes, hipMemcpyHostToDevice) : hipMemset(q, 0, bytes)) != hipSuccess) return nullptr;
            return q;
        }
    } dev;
    const size_t units = (size_t) S * NG * 2;
    void *d_st = dev.up(st.data(), sizeof(HxStream) * S), *d_prm = dev.up(prm.data(), sizeof(HxParams) * ncls), *d_gt = dev.up(&gt_host[0], sizeof(HxGlobalTabs));
    void *d_rt = dev.up(&rt_host[0], sizeof(HxReconTabs)), *d_ixq = dev.up(ixq, sizeof(short) * 576 * units), *d_sgn = dev.up(sgn, sizeof(unsigned) * HX_SGN_WORDS * units);
    void *d_seg = dev.up(seg, sizeof(HxSegOut) * units), *d_rec = dev.up(rec, sizeof(HxFrameDebug) * (size_t) S * (NG / 2));
    void *d_state = dev.up(state, sizeof(float) * HX_RECON_STATE_FLOATS * (size_t) S), *d_hyb = dev.up(hyb, sizeof(float) * 576 * units);
    void *d_tails = dev.up(nullptr, sizeof(float) * HX_RECON_TAIL_FLOATS * (size_t) S), *d_out = dev.up(out, sizeof(float) * (size_t) S * row);
    void *d_nfr = nfr ? dev.up(nfr, sizeof(int) * S) : nullptr;
    if (!d_st || !d_prm || !d_gt || !d_rt || !d_ixq || !d_sgn || !d_seg || !d_rec || !d_state || !d_hyb || !d_tails || !d_out || (nfr && !d_nfr)) {
        set_err("hipMalloc or upload failed");
        return -1;
    }
    if (launch_recon(nullptr, (const HxStream *) d_st, (const HxParams *) d_prm, (const HxGlobalTabs *) d_gt, (const HxReconTabs *) d_rt, (const short *) d_ixq,
                     (const unsigned *) d_sgn, (const HxSegOut *) d_seg, (const HxFrameDebug *) d_rec, (float *) d_hyb, (float *) d_tails, (float *) d_state,
                     (float *) d_out, row, S, NG, (const int *) d_nfr) != 0) return -1;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(state, d_state, sizeof(float) * HX_RECON_STATE_FLOATS * (size_t) S, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hyb, d_hyb, sizeof(float) * 576 * units, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out, d_out, sizeof(float) * (size_t) S * row, hipMemcpyDeviceToHost));
    return 0;
}


// ---- hx_debug_spec: K4 on subband blocks of the caller's (tests only; include/hmp3_amd.h) ----
// What k_spec / k_spec_direct read of a call - the subband slots k_polyphase fills and k_detect's block types - comes from the
// caller; the kernels and their launch are the batch's (launch_spec), HxParams, HxGlobalTabs and HxStream staged as
// batch_create stages them.  Every block a wave will read is checked on the host first.

static int spec_refuse(long long s, int g, int ch, const char *field, const char *what)
{
    char msg[256];
    if (g < 0) snprintf(msg, sizeof msg, "hx_debug_spec: stream %lld: %s: %s", s, field, what);
    else if (ch < 0) snprintf(msg, sizeof msg, "hx_debug_spec: stream %lld granule %d: %s: %s", s, g, field, what);
    else snprintf(msg, sizeof msg, "hx_debug_spec: stream %lld granule %d channel %d: %s: %s", s, g, ch, field, what);
    set_err("%s", msg);
    return -1;
}

extern "C" int hx_debug_spec(int device, const HX_E_CONTROL *ec, int ncls, const int *cls, int S, int NG, const int *nfr, int direct,
                             const float *sb, const unsigned char *bt, float *xr, float *etab, float *thr, int *msbase)
{
    if (!ec || !cls || !sb || !bt || !xr || !etab || !thr || !msbase) { set_err("null buffer"); return -1; }
    if (ncls <= 0 || S <= 0 || NG <= 0 || (NG & 1) || (direct != 0 && direct != 1)) { set_err("bad arguments"); return -1; }
    if ((long long) S * NG > (1LL << 16)) { set_err("hx_debug_spec takes at most 65536 granule positions (S * NG) per call"); return -1; }
    std::vector<HxParams> prm(ncls + 1);        // (one more: k_spec reads a spreading row in 16-byte pieces, up to 60 bytes past its end)
    for (int k = 0; k < ncls; k++)
        if (!hx_resolve((const HxControl *) (ec + k), &prm[k])) { set_err("configuration rejected"); return -1; }
    memset((void *) &prm[ncls], 0, sizeof(HxParams));
    for (int s = 0; s < S; s++) if (cls[s] < 0 || cls[s] >= ncls) { set_err("a stream's class is out of range"); return -1; }
    if (check_counts_arg(nfr, S, NG / 2, 0) != 0) return -1;
    const int SG = NG + 1;
    for (long long s = 0; s < S; s++) {
        const int ng = nfr ? 2 * nfr[s] : NG;
        for (int g = 0; g < ng; g++)
            if (bt[s * NG + g] > 3) return spec_refuse(s, g, -1, "bt", "a block type outside 0 .. 3");
        // (the first-generation allocator's streams run no detector: k_detect hands their granules type 0, and their metric is the long one's)
        for (int g = 0; g < ng && prm[cls[s]].alloc1; g++)
            if (bt[s * NG + g] != 0) return spec_refuse(s, g, -1, "bt", "a block type other than 0 in a stream of the first-generation allocator, which codes long blocks only");
        for (int ch = 0; ch < 2 && ng > 0; ch++)
            for (int g = 0; g <= ng; g++) {     // (block g is read by granules g - 1 and g)
                const float *v = sb + ((s * 2 + ch) * SG + g) * 576;
                for (int i = 0; i < 576; i++) {
                    if (!std::isfinite(v[i])) return spec_refuse(s, g, ch, "sb", "a sample that is not finite");
                    if (std::fabs(v[i]) > HX_SPEC_SAMPLE_MAX) return spec_refuse(s, g, ch, "sb", "a sample above HX_SPEC_SAMPLE_MAX in magnitude");
                }
            }
    }
    std::vector<HxGlobalTabs> gt_host(1);
    hx_global_tabs(&gt_host[0]);
    std::vector<HxStream> st(S);
    for (int s = 0; s < S; s++) hx_stream_reset(&prm[cls[s]], cls[s], &st[s]);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_err("no HIP device available: the encoder has no CPU fallback"); return -1; }
    if (device < 0 || device >= ndev) { set_err("device index out of range"); return -1; }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { set_err("device is %s: this library runs on gfx950 (MI355X) only", prop.gcnArchName); return -1; }
    HIPCHK(hipSetDevice(device));
    struct Dev {        // device copies: everything is released on every way out
        std::vector<void *> mem;
        ~Dev() { for (void *p : mem) (void) hipFree(p); }
        void *up(const void *src, size_t bytes)
        {
            void *q = nullptr;
            if (hipMalloc(&q, bytes) != hipSuccess) return nullptr;
            mem.push_back(q);
            if (hipMemcpy(q, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
            return q;
        }
    } dev;
    const size_t units = (size_t) S * NG;
    void *d_st = dev.up(st.data(), sizeof(HxStream) * S), *d_prm = dev.up(prm.data(), sizeof(HxParams) * (ncls + 1)), *d_gt = dev.up(&gt_host[0], sizeof(HxGlobalTabs));
    void *d_sb = dev.up(sb, sizeof(float) * 576 * 2 * (size_t) S * SG), *d_bt = dev.up(bt, units);
    void *d_xr = dev.up(xr, sizeof(float) * 1152 * units), *d_etab = dev.up(etab, sizeof(float) * 128 * units), *d_thr = dev.up(thr, sizeof(float) * 128 * units);
    void *d_ms = dev.up(msbase, sizeof(int) * units), *d_nfr = nfr ? dev.up(nfr, sizeof(int) * S) : nullptr;
    if (!d_st || !d_prm || !d_gt || !d_sb || !d_bt || !d_xr || !d_etab || !d_thr || !d_ms || (nfr && !d_nfr)) { set_err("hipMalloc or upload failed"); return -1; }
    if (launch_spec(nullptr, direct != 0, (const float *) d_sb, (const HxStream *) d_st, (const HxParams *) d_prm, (const HxGlobalTabs *) d_gt,
                    (const unsigned char *) d_bt, (float *) d_xr, (float *) d_etab, (float *) d_thr, (int *) d_ms, S, NG, SG, (const int *) d_nfr) != 0) return -1;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(xr, d_xr, sizeof(float) * 1152 * units, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(etab, d_etab, sizeof(float) * 128 * units, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(thr, d_thr, sizeof(float) * 128 * units, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(msbase, d_ms, sizeof(int) * units, hipMemcpyDeviceToHost));
    return 0;
}


// ---- hx_debug_count: the stream walk's quantiser and Huffman counter on records of the caller's (tests only; include/hmp3_amd.h) ----
// The kernels are the walk units' twins (k_debug_count_*, hx_alloc3.inc).  Every record is checked on the host first: the
// quantiser's result is worked out here the way the kernel will (same expression, same tables), and what the counter would
// then be handed must be something the walk can hand it - so no table index, line index or packed 16-bit sum of the kernel
// sees a value it was not written for.

static int count_refuse(long long r, int ch, const char *what)
{
    char msg[256];
    if (ch >= 0) snprintf(msg, sizeof msg, "record %lld channel %d: %s", r, ch, what);
    else snprintf(msg, sizeof msg, "record %lld: %s", r, what);
    set_err("%s", msg);
    return -1;
}

#define HX_IX_MAX 8206      // the largest value the format codes: 15 + 2^13 - 1

// one line through the long-block quantiser (quant_lines, hx_alloc.hip): -1 = not a value the counter takes
static int count_quant_line(const HxParams &p, const HxGlobalTabs &gt, int gsf, float x34, int tab, bool short_first)
{
    if (!(x34 >= 0.0f) || !(x34 <= 3.0e38f)) return -1;
    const float igain = p.look_34igain[gsf];
    float q;
    if (tab) {
        const float t = igain * x34 + (0.5f - 0.4375f);
        if (!(t < 16384.0f)) return -1;
        const int iq = std::max(std::min((int) t, 31), 0);
        q = t - ((short_first && iq == 0) ? -.30f : gt.quant_off[iq]);
    } else q = igain * x34 + (0.5f - 0.0946f);
    if (!(q < 16384.0f)) return -1;
    const int v = (int) q;
    return (v < 0 || v > HX_IX_MAX) ? -1 : v;
}

// what count_bits_ch makes of a channel's band maxima and lines before it reads a pair: where the big values end, how many
// count1 quadruples follow
static void count_split(const HxParams &p, int bt, int ncb, const int *ixmax, const int *ix, int *nbig_out, int *nquads_out)
{
    int i;
    for (i = ncb - 1; i >= 0; i--) if (ixmax[i] > 0) break;
    int cb3 = i + 1;
    for (; i >= 0; i--) if (ixmax[i] > 1) break;
    int cb2 = i + 1;
    if (bt == 0) { if (cb2 < 2) { cb2 = 2; if (cb3 < cb2) cb3 = cb2; } }
    else { cb2 = std::max(cb2, 8); cb3 = std::max(cb3, cb2); }
    int j2 = p.startBand_l[cb2 - 1], j3 = p.startBand_l[cb3 - 1];
    for (int j = p.startBand_l[cb2 - 1]; j < p.startBand_l[cb2]; j++) if (ix[j] > 1) j2 = j;
    for (int j = p.startBand_l[cb3 - 1]; j < p.startBand_l[cb3]; j++) if (ix[j] > 0) j3 = j;
    int nbig = (j2 + 2) & ~1;
    nbig = std::max(nbig, p.startBand_l[bt == 0 ? 2 : 8]);
    int nquads = (j3 + 4 - nbig) >> 2;
    if (bt != 0) nquads = std::max(nquads, 0);
    *nbig_out = nbig; *nquads_out = nquads;
}

static int check_count_long(const HxParams &p, const HxGlobalTabs &gt, bool slim, int mode, long long r, const int *h,
                            const int *ix_in, const int *ixmax_in, const float *x34, const int *gsf)
{
    const int bt = h[HX_DCH_BT], nchan = h[HX_DCH_NCHAN], opt = h[HX_DCH_OPT], zero21 = h[HX_DCH_ZERO21];
    const bool quant = mode != HX_DC_COUNT;
    if (bt != 0 && bt != 1 && bt != 3) return count_refuse(r, -1, "block type is not 0, 1 or 3");
    if (nchan != 1 && nchan != 2) return count_refuse(r, -1, "channel count is not 1 or 2");
    if (quant ? (opt != 0 && opt != 1 && opt != 3) || (zero21 != 0 && zero21 != 1) : (opt != 0 || zero21 != 0))
        return count_refuse(r, -1, quant ? "opt is not 0, 1 or 1 | 2, or zero21 not 0 or 1" : "opt and zero21 are the quantising modes'");
    for (int k = HX_DCH_NBMAX1 + 1; k < HX_DCH_WORDS; k++) if (h[k]) return count_refuse(r, -1, "a spare header word is not zero");
    int ix[2][576 + 4], ixmax[2][22];
    for (int c = 0; c < 2; c++) {
        for (int j = 0; j < 576; j++) {
            ix[c][j] = ix_in[576 * c + j];
            if (ix[c][j] < 0 || ix[c][j] > HX_IX_MAX) return count_refuse(r, c, "a line outside 0 .. 8206");
        }
        for (int b = 0; b < 22; b++) {
            ixmax[c][b] = ixmax_in[22 * c + b];
            if (ixmax[c][b] < 0 || ixmax[c][b] > HX_IX_MAX) return count_refuse(r, c, "a band maximum outside 0 .. 8206");
        }
    }
    for (int c = 0; c < nchan; c++) {
        const int ncb = h[HX_DCH_NCB0 + c];
        if (ncb < 1 || ncb > 22) return count_refuse(r, c, "ncb outside 1 .. 22");
        if (!quant) {
            if (h[HX_DCH_NSF0 + c] || h[HX_DCH_NBMAX0 + c]) return count_refuse(r, c, "nsf and nbmax are the quantising modes'");
            continue;
        }
        const int nsf = h[HX_DCH_NSF0 + c], nl = h[HX_DCH_NBMAX0 + c];
        if (nsf < 1 || nsf > 22) return count_refuse(r, c, "nsf outside 1 .. 22");
        if (nl != p.startBand_l[nsf]) return count_refuse(r, c, "nbmax is not the first line behind band nsf - 1");
        // lines at and past nbmax: the low-footprint layout writes zeros there unless opt & 2 (quant_lines), the others leave
        // them alone, and the walk never hands over anything there but zeros and, under opt & 2, band 21 of an earlier -HF pass
        const bool cleared = slim && !(opt & 2);
        for (int j = nl; j < 576; j++) {
            if (cleared) ix[c][j] = 0;
            else if (ix[c][j] != 0 && !((opt & 2) && j >= p.startBand_l[21])) return count_refuse(r, c, "a line at or past nbmax is not zero (band 21 under opt & 2 may be)");
        }
        for (int b = 0; b < 22; b++) {
            if (gsf[22 * c + b] < 0 || gsf[22 * c + b] > 127) return count_refuse(r, c, "a gain step outside 0 .. 127");
            if (b < nsf) ixmax[c][b] = 0;
        }
        for (int j = 0; j < nl; j++) {
            const int b = p.band_of_line[j];
            const int v = count_quant_line(p, gt, gsf[22 * c + b], x34[576 * c + j], opt & 1, false);
            if (v < 0) return count_refuse(r, c, "a line that is not a finite magnitude, or that quantises above 8206");
            ix[c][j] = v;
            ixmax[c][b] = std::max(ixmax[c][b], v);
        }
    }
    if (quant && zero21) ixmax[0][21] = 0;
    for (int c = 0; c < nchan; c++) {
        // a band's maximum covers its lines: the tables are picked from the maxima, and a line above its table's range
        // would index past the table
        for (int j = 0; j < 576; j++) {
            const int b = p.band_of_line[j];
            if (ix[c][j] > ixmax[c][b] && !(quant && zero21 && c == 0 && b == 21)) return count_refuse(r, c, "a line above its band's maximum");
        }
        int nbig, nquads;
        count_split(p, bt, h[HX_DCH_NCB0 + c], ixmax[c], ix[c], &nbig, &nquads);
        const int end = nbig + 4 * std::max(nquads, 0);
        // The last quadruple reaches lines 576 and 577 where the last non-zero line is 574 or 575 and nbig = 2 mod 4.
        // Channel 0's are then channel 1's first two lines, in the reference's arrays (CMp3Enc::ix[2][576]) as in both LDS
        // layouts, and a record may say so.  Channel 1's would be the first bytes of the reference's sign array, a mono
        // stream's whatever channel 1's lines last held.  No stream gets there, on either channel: a band is quantised
        // only below nsf <= 21 (L3init_sfbl_limit2 caps it; band 20 ends at line 549 at the latest), and band
        // 21 only under -HF, which the reference keeps to 44.1 and 48 kHz and cuts to 100 lines there (bitallo3.cpp:327-331:
        // lines up to 517 and 483), and everything above stays zero.  So there is nothing to define for channel 1: such a
        // record is refused, and so is a mono one.
        if (end > 576) {
            if (c == 1 || nchan == 1) return count_refuse(r, c, "the last count1 quadruple reaches past line 575 with no second channel's lines behind it");
            if (mode == HX_DC_QUANT_COUNT) return count_refuse(r, c, "the last count1 quadruple reads channel 1's lines while the helper wave quantises them: the walk goes unfused there");
            ix[0][576] = ix[1][0]; ix[0][577] = ix[1][1];       // (as channel 1's quantiser leaves them, where it runs)
        }
        for (int j = nbig; j < end; j++) if (ix[c][j] > 1) return count_refuse(r, c, "a count1 quadruple holds a value above 1");
    }
    return 0;
}

static int check_count_short(const HxParams &p, const HxGlobalTabs &gt, int mode, long long r, const int *h,
                             const int *ix_in, const int *ixmax_in, const float *x34, const int *gsf)
{
    const int nchan = h[HX_DCH_NCHAN], opt = h[HX_DCH_OPT];
    const bool quant = mode == HX_DC_SHORT;
    if (nchan != 1 && nchan != 2) return count_refuse(r, -1, "channel count is not 1 or 2");
    if (opt != 0 && !(quant && opt == 1)) return count_refuse(r, -1, "opt is not 0 or 1, or set where nothing is quantised");
    for (int k = 0; k < HX_DCH_WORDS; k++) if (k != HX_DCH_NCHAN && k != HX_DCH_OPT && h[k]) return count_refuse(r, -1, "a header word a short record does not use is not zero");
    for (int c = 0; c < 2; c++)             // (s_do_quant quantises both channels' lines, whatever the channel count)
        for (int w = 0; w < 3; w++) {
            int bmax[16] = {0};
            for (int j = 0; j < 192; j++) {
                int v = ix_in[(3 * c + w) * 192 + j];
                if (v < 0 || v > HX_IX_MAX) return count_refuse(r, c, "a line outside 0 .. 8206");
                if (j >= p.nbmax_s) continue;
                const int b = p.sband_of_line[j];
                if (quant) {
                    const int g = gsf[(3 * c + w) * 16 + b];
                    if (g < 0 || g > 127) return count_refuse(r, c, "a gain step outside 0 .. 127");
                    v = count_quant_line(p, gt, g, x34[(3 * c + w) * 192 + j], opt, true);
                    if (v < 0) return count_refuse(r, c, "a line that is not a finite magnitude, or that quantises above 8206");
                }
                bmax[b] = std::max(bmax[b], v);
            }
            for (int b = 0; b < 16; b++) {
                const int m = ixmax_in[(3 * c + w) * 16 + b];
                if (m < 0 || m > HX_IX_MAX) return count_refuse(r, c, "a band maximum outside 0 .. 8206");
                if (!quant && c < nchan && m < bmax[b]) return count_refuse(r, c, "a line above its band's maximum");
            }
        }
    return 0;
}

extern "C" int hx_debug_count(int device, const HX_E_CONTROL *ec, const char *unit, int mode, int n, const int *hdr, int *ix, int *ixmax,
                              const float *x34, const int *gsf, int *out)
{
    if (!ec || !unit || !hdr || !ix || !ixmax || !out) { set_err("null buffer"); return -1; }
    if (mode < 0 || mode >= HX_DC_MODES) { set_err("hx_debug_count: no such mode"); return -1; }
    const bool quant = mode == HX_DC_QUANT_COUNT || mode == HX_DC_QUANT_THEN_COUNT || mode == HX_DC_SHORT;
    const bool shortm = mode == HX_DC_SHORT || mode == HX_DC_SHORT_COUNT;
    if (quant && (!x34 || !gsf)) { set_err("null buffer"); return -1; }
    if (n <= 0 || n > HX_DEBUG_COUNT_MAX) { set_err("hx_debug_count takes 1 .. 16384 records per call"); return -1; }
    static const char *const units[5] = {"k_alloc", "k_alloc_slim", "k_alloc_lsf", "k_alloc1", "k_alloc1_lsf"};
    int u = -1;
    for (int k = 0; k < 5; k++) if (!strcmp(unit, units[k])) u = k;
    if (u < 0) { set_err("hx_debug_count: no stream-walk unit named %s", unit); return -1; }
    std::vector<HxParams> prm(1);
    if (!hx_resolve((const HxControl *) ec, &prm[0])) { set_err("configuration rejected"); return -1; }
    std::vector<HxGlobalTabs> gt(1);
    hx_global_tabs(&gt[0]);
    // the unit that walks a stream of this control (hx_batch_create: kind = 2 * first-generation + MPEG-2)
    const int kind = 2 * (prm[0].alloc1 ? 1 : 0) + (prm[0].h_id ? 0 : 1);
    static const int unit_kind[5] = {0, 0, 1, 2, 3};
    if (unit_kind[u] != kind) { set_err("hx_debug_count: %s does not run streams of this control", unit); return -1; }
    if (u == 1 && !hx_slim_tables_ok(&prm[0], &gt[0])) { set_err("hx_debug_count: the host's tables do not have the structure k_alloc_slim derives them from"); return -1; }
    const int nband = shortm ? 48 : 22;
    for (long long r = 0; r < n; r++) {
        const int *h = hdr + r * HX_DCH_WORDS;
        const int rc = shortm ? check_count_short(prm[0], gt[0], mode, r, h, ix + r * 1152, ixmax + r * 96, quant ? x34 + r * 1152 : nullptr, quant ? gsf + r * 96 : nullptr)
                              : check_count_long(prm[0], gt[0], u == 1, mode, r, h, ix + r * 1152, ixmax + r * 44, quant ? x34 + r * 1152 : nullptr, quant ? gsf + r * 44 : nullptr);
        if (rc != 0) return -1;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_err("no HIP device available: the encoder has no CPU fallback"); return -1; }
    if (device < 0 || device >= ndev) { set_err("device index out of range"); return -1; }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { set_err("device is %s: this library runs on gfx950 (MI355X) only", prop.gcnArchName); return -1; }
    HIPCHK(hipSetDevice(device));
    struct Dev {
        std::vector<void *> mem;
        ~Dev() { for (void *p : mem) (void) hipFree(p); }
        void *up(const void *src, size_t bytes)
        {
            void *q = nullptr;
            if (hipMalloc(&q, bytes ? bytes : 16) != hipSuccess) return nullptr;
            mem.push_back(q);
            if (src ? hipMemcpy(q, src, bytes, hipMemcpyHostToDevice) != hipSuccess : hipMemset(q, 0, bytes) != hipSuccess) return nullptr;
            return q;
        }
    } dev;
    std::vector<HxStream> st(1);
    hx_stream_reset(&prm[0], 0, &st[0]);
    const size_t N = (size_t) n;
    AllocArgs a = {};
    HxCountArgs c = {};
    a.st = (HxStream *) dev.up(st.data(), sizeof(HxStream));
    a.prm = (const HxParams *) dev.up(prm.data(), sizeof(HxParams));
    a.gt = (const HxGlobalTabs *) dev.up(gt.data(), sizeof(HxGlobalTabs));
    a.done_counter = (int *) dev.up(nullptr, sizeof(int) * HX_CNT_WORDS);
    a.S = 1; a.NG = 2; a.npos = 1;
    c.mode = mode; c.n = n; c.nband = nband;
    c.hdr = (const int *) dev.up(hdr, sizeof(int) * HX_DCH_WORDS * N);
    c.ix = (int *) dev.up(ix, sizeof(int) * 1152 * N);
    c.ixmax = (int *) dev.up(ixmax, sizeof(int) * 2 * nband * N);
    c.x34 = quant ? (const float *) dev.up(x34, sizeof(float) * 1152 * N) : nullptr;
    c.gsf = quant ? (const int *) dev.up(gsf, sizeof(int) * 2 * nband * N) : nullptr;
    c.out = (int *) dev.up(nullptr, sizeof(int) * HX_DCO_WORDS * N);
    if (!a.st || !a.prm || !a.gt || !a.done_counter || !c.hdr || !c.ix || !c.ixmax || (quant && (!c.x34 || !c.gsf)) || !c.out) { set_err("hipMalloc or upload failed"); return -1; }
    const dim3 grid((unsigned) n), block(128);
    if (u == 0) LAUNCH(k_debug_count, grid, block, 0, a, c);
    else if (u == 1) LAUNCH(k_debug_count_slim, grid, block, 0, a, c);
    else if (u == 2) LAUNCH(k_debug_count_lsf, grid, block, 0, a, c);
    else if (u == 3) LAUNCH(k_debug_count_a1, grid, block, 0, a, c);
    else LAUNCH(k_debug_count_a1_lsf, grid, block, 0, a, c);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(ix, c.ix, sizeof(int) * 1152 * N, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ixmax, c.ixmax, sizeof(int) * 2 * nband * N, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out, c.out, sizeof(int) * HX_DCO_WORDS * N, hipMemcpyDeviceToHost));
    return 0;
}

// ---- hx_debug_seek: the stream walk's gain search and inverse_sf2 on records of the caller's (tests only; include/hmp3_amd.h) ----
// The kernels are hx_debug_count's (the noise modes of k_debug_count_*, hx_alloc3.inc).  One rule per field, checked for every
// record before anything is launched; what a value indexes on the device - gain tables, band tables, the lanes' runs - stays
// inside its bounds under these rules (hx_types.h states the one for the gain steps).

static int seek_refuse(long long r, int ch, int b, const char *field, const char *rule)
{
    char msg[256];
    if (b >= 0) snprintf(msg, sizeof msg, "record %lld channel %d band %d: %s %s", r, ch, b, field, rule);
    else if (ch >= 0) snprintf(msg, sizeof msg, "record %lld channel %d: %s %s", r, ch, field, rule);
    else snprintf(msg, sizeof msg, "record %lld: %s %s", r, field, rule);
    set_err("%s", msg);
    return -1;
}

static int check_seek_record(const HxParams &p, bool isf2, long long r, const int *h, const float *xr, const float *x34, const int *ix,
                             const int *band, const float *x34max)
{
    const int nchan = h[HX_DSH_NCHAN];
    if (nchan != 1 && nchan != 2) return seek_refuse(r, -1, -1, "nchan", "is not 1 or 2");
    if (h[HX_DSH_NSFS]) return seek_refuse(r, -1, -1, "the short-block band count", "is not zero: neither function reads it");
    if (h[HX_DSH_HF]) return seek_refuse(r, -1, -1, "the -HF count", "is not zero: neither function reads it");
    for (int k = HX_DSH_HF + 1; k < HX_DSH_WORDS; k++) if (h[k]) return seek_refuse(r, -1, -1, "a spare header word", "is not zero");
    // the bands that have lanes: the runs are cut for the class's measured bands (hx_host.cpp band_runs)
    const int nbcls = std::max(p.nsf[0], p.nchan == 2 ? p.nsf[1] : 0);
    for (int c = 0; c < 2; c++) {
        const int nsf = h[HX_DSH_NSF0 + c], nl = h[HX_DSH_NBMAX0 + c], G = h[HX_DSH_G0 + c], scale = h[HX_DSH_SCALE0 + c];
        if (c >= nchan) {
            if (nsf) return seek_refuse(r, c, -1, "nsf", "of a channel the record does not have is not zero");
            if (nl) return seek_refuse(r, c, -1, "nbmax", "of a channel the record does not have is not zero");
        } else {
            if (nsf < 1 || nsf > nbcls) return seek_refuse(r, c, -1, "nsf", "is outside 1 .. the class's band count");
            if (nl != p.startBand_l[nsf]) return seek_refuse(r, c, -1, "nbmax", "is not the first line behind band nsf - 1");
        }
        if (isf2 ? (G < 0 || G > 255) : G != 0) return seek_refuse(r, c, -1, "G", isf2 ? "is outside 0 .. 255" : "is inverse_sf2's: not zero");
        if (isf2 ? (scale != 0 && scale != 1) : scale != 0) return seek_refuse(r, c, -1, "scale", isf2 ? "is not 0 or 1" : "is inverse_sf2's: not zero");
        for (int j = 0; j < 576; j++) {
            const int b = p.band_of_line[j];
            if (!(fabsf(xr[576 * c + j]) <= 3.0e38f)) return seek_refuse(r, c, b, "xr", "holds a line that is not finite");
            if (isf2) { if (ix[576 * c + j] < 0 || ix[576 * c + j] > HX_IX_MAX) return seek_refuse(r, c, b, "ix", "holds a line outside 0 .. 8206"); }
            else if (!(x34[576 * c + j] >= 0.0f && x34[576 * c + j] <= HX_DS_X34_MAX)) return seek_refuse(r, c, b, "x34", "holds a line outside 0 .. 2^28");
        }
        for (int b = 0; b < 22; b++) {
            const int *w = band + (22 * c + b) * HX_DSB_WORDS;
            const int j0 = p.startBand_l[b], j1 = b < 21 ? p.startBand_l[b + 1] : 576;
            if (isf2) {
                int m = 0;
                for (int j = j0; j < j1; j++) m = std::max(m, ix[576 * c + j]);
                if (w[HX_DSB_IXMAX] != m) return seek_refuse(r, c, b, "ixmax", "is not the maximum of the band's lines");
                if (w[HX_DSB_LO] < 0 || w[HX_DSB_LO] > 255) return seek_refuse(r, c, b, "lo", "is outside 0 .. 255");
                if (w[HX_DSB_UP] < w[HX_DSB_LO] || w[HX_DSB_UP] > 255) return seek_refuse(r, c, b, "up", "is below lo or above 255");
                if (w[HX_DSB_SF] < 0 || w[HX_DSB_SF] > 255) return seek_refuse(r, c, b, "sf", "is outside 0 .. 255");
                for (int k = HX_DSB_IXMAX + 1; k < HX_DSB_WORDS; k++) if (w[k]) return seek_refuse(r, c, b, "a spare band word", "is not zero");
            } else {
                float m = 0.0f;
                for (int j = j0; j < j1; j++) m = std::max(m, x34[576 * c + j]);
                // (noise_band_needs_pow picks the sweep's route from it)
                if (!(x34max[22 * c + b] == m)) return seek_refuse(r, c, b, "x34max", "is not the maximum of the band's x34");
                if (abs(w[HX_DSB_NT]) > HX_DS_INT_MAX) return seek_refuse(r, c, b, "NT", "is outside -2^20 .. 2^20");
                if (abs(w[HX_DSB_NOISE0]) > HX_DS_INT_MAX) return seek_refuse(r, c, b, "Noise0", "is outside -2^20 .. 2^20");
                if (abs(w[HX_DSB_NTADJUST]) > HX_DS_INT_MAX) return seek_refuse(r, c, b, "NTadjust", "is outside -2^20 .. 2^20");
                if (w[HX_DSB_GSF] < 0 || w[HX_DSB_GSF] > HX_DS_GSF_MAX) return seek_refuse(r, c, b, "gsf", "is outside 0 .. 107: 20 steps up from it must stay inside the gain tables");
                if (w[HX_DSB_GZERO] < 0 || w[HX_DSB_GZERO] > 127) return seek_refuse(r, c, b, "gzero", "is outside 0 .. 127");
                for (int k = HX_DSB_NTADJUST + 1; k < HX_DSB_WORDS; k++) if (w[k]) return seek_refuse(r, c, b, "a spare band word", "is not zero");
            }
        }
    }
    return 0;
}

extern "C" int hx_debug_seek(int device, const HX_E_CONTROL *ec, const char *unit, int mode, int strict_sums, int n, const int *hdr,
                             const float *xr, const float *x34, const int *ix, const int *band, const float *x34max, int *out)
{
    if (!ec || !unit || !hdr || !xr || !band || !out) { set_err("null buffer"); return -1; }
    if (mode != 0 && mode != 1) { set_err("hx_debug_seek: no such mode"); return -1; }
    const bool isf2 = mode == 1;
    if (isf2 ? !ix : (!x34 || !x34max)) { set_err("null buffer"); return -1; }
    if (strict_sums != 0 && strict_sums != 1) { set_err("hx_debug_seek: strict_sums is 0 or 1"); return -1; }
    if (n <= 0 || n > HX_DEBUG_COUNT_MAX) { set_err("hx_debug_seek takes 1 .. 16384 records per call"); return -1; }
    static const char *const units[5] = {"k_alloc", "k_alloc_slim", "k_alloc_lsf", "k_alloc1", "k_alloc1_lsf"};
    int u = -1;
    for (int k = 0; k < 5; k++) if (!strcmp(unit, units[k])) u = k;
    if (u < 0) { set_err("hx_debug_seek: no stream-walk unit named %s", unit); return -1; }
    if (u >= 3) { set_err("hx_debug_seek: %s is a first-generation unit, which runs neither seek_actual nor inverse_sf2", unit); return -1; }
    std::vector<HxParams> prm(1);
    if (!hx_resolve((const HxControl *) ec, &prm[0])) { set_err("configuration rejected"); return -1; }
    std::vector<HxGlobalTabs> gt(1);
    hx_global_tabs(&gt[0]);
    const int kind = 2 * (prm[0].alloc1 ? 1 : 0) + (prm[0].h_id ? 0 : 1);
    static const int unit_kind[3] = {0, 0, 1};
    if (unit_kind[u] != kind) { set_err("hx_debug_seek: %s does not run streams of this control", unit); return -1; }
    if (u == 1 && !hx_slim_tables_ok(&prm[0], &gt[0])) { set_err("hx_debug_seek: the host's tables do not have the structure k_alloc_slim derives them from"); return -1; }
    for (long long r = 0; r < n; r++)
        if (check_seek_record(prm[0], isf2, r, hdr + r * HX_DSH_WORDS, xr + r * 1152, isf2 ? nullptr : x34 + r * 1152, isf2 ? ix + r * 1152 : nullptr,
                              band + r * 44 * HX_DSB_WORDS, isf2 ? nullptr : x34max + r * 44) != 0) return -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_err("no HIP device available: the encoder has no CPU fallback"); return -1; }
    if (device < 0 || device >= ndev) { set_err("device index out of range"); return -1; }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { set_err("device is %s: this library runs on gfx950 (MI355X) only", prop.gcnArchName); return -1; }
    HIPCHK(hipSetDevice(device));
    struct Dev {
        std::vector<void *> mem;
        ~Dev() { for (void *p : mem) (void) hipFree(p); }
        void *up(const void *src, size_t bytes)
        {
            void *q = nullptr;
            if (hipMalloc(&q, bytes ? bytes : 16) != hipSuccess) return nullptr;
            mem.push_back(q);
            if (src ? hipMemcpy(q, src, bytes, hipMemcpyHostToDevice) != hipSuccess : hipMemset(q, 0, bytes) != hipSuccess) return nullptr;
            return q;
        }
    } dev;
    std::vector<HxStream> st(1);
    hx_stream_reset(&prm[0], 0, &st[0]);
    const size_t N = (size_t) n;
    AllocArgs a = {};
    HxCountArgs c = {};
    a.st = (HxStream *) dev.up(st.data(), sizeof(HxStream));
    a.prm = (const HxParams *) dev.up(prm.data(), sizeof(HxParams));
    a.gt = (const HxGlobalTabs *) dev.up(gt.data(), sizeof(HxGlobalTabs));
    a.done_counter = (int *) dev.up(nullptr, sizeof(int) * HX_CNT_WORDS);
    a.S = 1; a.NG = 2; a.npos = 1;
    a.strict_sums = strict_sums;
    c.mode = HX_DS_SEEK + mode; c.n = n; c.nband = 22;
    c.hdr = (const int *) dev.up(hdr, sizeof(int) * HX_DSH_WORDS * N);
    c.xr = (const float *) dev.up(xr, sizeof(float) * 1152 * N);
    c.band = (const int *) dev.up(band, sizeof(int) * 44 * HX_DSB_WORDS * N);
    c.x34 = isf2 ? nullptr : (const float *) dev.up(x34, sizeof(float) * 1152 * N);
    c.x34max = isf2 ? nullptr : (const float *) dev.up(x34max, sizeof(float) * 44 * N);
    c.ix = isf2 ? (int *) dev.up(ix, sizeof(int) * 1152 * N) : nullptr;
    c.out = (int *) dev.up(nullptr, sizeof(int) * HX_DSO_WORDS * N);
    if (!a.st || !a.prm || !a.gt || !a.done_counter || !c.hdr || !c.xr || !c.band || (isf2 ? !c.ix : (!c.x34 || !c.x34max)) || !c.out) { set_err("hipMalloc or upload failed"); return -1; }
    const dim3 grid((unsigned) n), block(128);
    if (u == 0) LAUNCH(k_debug_count, grid, block, 0, a, c);
    else if (u == 1) LAUNCH(k_debug_count_slim, grid, block, 0, a, c);
    else LAUNCH(k_debug_count_lsf, grid, block, 0, a, c);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, c.out, sizeof(int) * HX_DSO_WORDS * N, hipMemcpyDeviceToHost));
    return 0;
}
