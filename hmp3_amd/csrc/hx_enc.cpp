// hx_enc.cpp - the CMp3Enc-compatible single-stream encoder of the C ABI (include/hmp3_amd.h): a batch of one, one frame
// per call, replayed from a HIP graph; and the encode control of a converted source (src_encode_control), which the
// converting batches share.  Launches no kernel itself: built by the host compiler.
#include <stddef.h>
#include <chrono>
#include <atomic>
#include <mutex>
#include <shared_mutex>
#include "hx_rt.h"

// While a stream of the process is being captured - in thread-local mode too - the runtime refuses every other thread's
// hipDeviceSynchronize (hipErrorStreamCaptureUnsupported) and null-stream calls such as hipMemcpy
// (hipErrorStreamCaptureImplicit), and the refused call invalidates the capture.  The plain calls, init and destroy make
// such calls, so encoders driven from threads of their own would fail each other's calls and lose their graphs: an
// encoder records its graph alone (exclusive), and everything else an encoder does on the device shares the lock.
static std::shared_mutex g_record_lock;
using EncUse = std::shared_lock<std::shared_mutex>;
using EncRecord = std::unique_lock<std::shared_mutex>;

struct hx_enc {
    int device = 0;
    hx_batch *b = nullptr;
    HxParams p;
    int src_bits = 0, src_float = 0;
    int src_chan = 2;                   // channels of the caller's PCM (2 with mono_convert: down-mixed to one)
    std::vector<unsigned char> outbuf;
    unsigned frames = 0, bytes = 0;
    int ave = 0;
    hx_src *src = nullptr;              // converter of the MP3_audio_encode entry points
    unsigned char *d_packet = nullptr;  // one reformatted frame (device), allocated on first *_Packet call
    int *d_packet_bytes = nullptr;
    // One call = one graph launch: the whole single-stream chain (PCM up, the pipeline's kernels, byte count / frame counter /
    // bitstream down) is recorded once into a HIP graph over page-locked staging buffers and replayed per call
    // (reference call being replaced: CMp3Enc::L3_audio_encode, mp3enc.cpp:2031-2073, and MP3_audio_encode, :2812-2866).
    hipStream_t gq = nullptr;
    unsigned char *d_encbuf = nullptr;  // device: [byte count | frame counter | ... HX_ENC_GRAPH_OFF | the call's bitstream]
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    float *h_pcm = nullptr;             // page-locked: one 1152-sample block, float at int16 scale
    unsigned char *h_out = nullptr;     // page-locked, coherent: [byte count | frame counter | sequence word | ... 256 | the call's bitstream], written by the packing workgroup
    int graph_state = 0;                // 0 = not built yet, 1 = ready, -1 = not available (disabled, or the build failed: plain calls)
    int plain_calls = 0;                // calls made the plain way since init (the first ones: they also load the kernels' code objects)
    int graph_calls = 0;                // calls replayed from the graph since init (hx_enc_debug_calls)
};
#define HX_ENC_GRAPH_OFF 256

static void enc_graph_drop(hx_enc *e)
{
    if (e->gexec) { hipGraphExecDestroy(e->gexec); e->gexec = nullptr; }
    if (e->graph) { hipGraphDestroy(e->graph); e->graph = nullptr; }
    if (e->gq) { hipStreamDestroy(e->gq); e->gq = nullptr; }
    if (e->d_encbuf) { hipFree(e->d_encbuf); e->d_encbuf = nullptr; }
    if (e->h_pcm) { hipHostFree(e->h_pcm); e->h_pcm = nullptr; }
    if (e->h_out) { hipHostFree(e->h_out); e->h_out = nullptr; }
    e->graph_state = 0;
    e->plain_calls = 0;
    e->graph_calls = 0;
}

extern "C" hx_enc *hx_enc_create(int device)
{
    hx_enc *e = new hx_enc;
    e->device = device;
    return e;
}

extern "C" void hx_enc_destroy(hx_enc *e)
{
    if (!e) return;
    EncUse use(g_record_lock);
    enc_graph_drop(e);
    if (e->d_packet) hipFree(e->d_packet);
    if (e->d_packet_bytes) hipFree(e->d_packet_bytes);
    hx_src_destroy(e->src);
    hx_batch_destroy(e->b);
    delete e;
}

extern "C" int hx_enc_L3_audio_encode_init(hx_enc *e, const HX_E_CONTROL *ec)
{
    EncUse use(g_record_lock);
    enc_graph_drop(e);
    if (e->b) { hx_batch_destroy(e->b); e->b = nullptr; }       // re-init is legal (mp3enc.cpp:267-272)
    int r = hx_resolve((const HxControl *) ec, &e->p);
    if (!r) { if (*hx_resolve_error()) set_err("configuration rejected: %s", hx_resolve_error()); else set_err("configuration rejected"); return 0; }
    e->b = hx_batch_create(e->device, 1, ec, 1, 1);
    if (!e->b) return 0;
    e->frames = e->bytes = 0; e->ave = 0;
    e->outbuf.assign((size_t) hx_batch_out_stride(e->b, 1) + 65536, 0);
    e->src_bits = 0;
    return r;
}

// Record the single-stream chain of e->b into a graph (see hx_enc).  Returns 0 when e->gexec is ready.
// The graph is the PCM's copy up from page-locked staging and the pipeline's kernels; the call's results - byte count, frame
// counter, bitstream - are written to page-locked host memory by the packing workgroup itself, which publishes a sequence word
// behind system-scope fences (hx_pack.hip, k_pack solo): the call polls that word.
static int enc_graph_build(hx_enc *e)
{
    hx_batch *b = e->b;
    HIPCHK(hipSetDevice(b->device));
    const long long stride = (long long) e->outbuf.size();
    const long long pbytes = 1152LL * b->nchan * (long long) sizeof(float);
    // allocated before the recording starts (no allocation inside one)
    if (dev_grow(b, b->d_in, b->in_cap, pbytes) != 0) return -1;
    HIPCHK(hipMalloc((void **) &e->d_encbuf, (size_t) (HX_ENC_GRAPH_OFF + stride)));
    HIPCHK(hipMemset(e->d_encbuf, 0, (size_t) (HX_ENC_GRAPH_OFF + stride)));
    HIPCHK(hipHostMalloc((void **) &e->h_pcm, (size_t) pbytes, hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **) &e->h_out, (size_t) (HX_ENC_GRAPH_OFF + stride + 16), hipHostMallocCoherent));
    memset(e->h_out, 0, (size_t) (HX_ENC_GRAPH_OFF + stride + 16));
    HIPCHK(hipMemcpy(e->h_out + 8, b->d_done + HX_CNT_STARTED, sizeof(int), hipMemcpyDeviceToHost));       // the sequence word as the device has it now
    HIPCHK(hipStreamCreateWithFlags(&e->gq, hipStreamNonBlocking));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipStreamBeginCapture(e->gq, hipStreamCaptureModeThreadLocal));
    int r = 0;
    Call c = {e->d_encbuf + HX_ENC_GRAPH_OFF, stride, reinterpret_cast<int *>(e->d_encbuf)};    // (no optional outputs: encode_one)
    c.rec_frames = reinterpret_cast<unsigned *>(e->d_encbuf) + 1;
    c.rec_host = e->h_out;
    c.recording = true;
    if (hipMemcpyAsync(b->d_in, e->h_pcm, (size_t) pbytes, hipMemcpyHostToDevice, e->gq) != hipSuccess) r = -1;
    if (!r) r = encode_checked(b, {b->d_in, true}, 1, c, e->gq, PASS_PLAIN);
    hipGraph_t g = nullptr;
    const hipError_t ce = hipStreamEndCapture(e->gq, &g);       // (always ended, also after a failure inside)
    if (r || ce != hipSuccess || !g) { if (g) hipGraphDestroy(g); (void) hipGetLastError(); set_err("recording the single-stream graph failed"); return -1; }
    e->graph = g;
    if (hipGraphInstantiate(&e->gexec, e->graph, nullptr, nullptr, 0) != hipSuccess) { (void) hipGetLastError(); set_err("hipGraphInstantiate failed"); return -1; }
    // (the recording has executed nothing; the counters the pass advanced on the host - launches, the carry's layout - are
    // the ones a real pass leaves behind, and the batch was not poisoned)
    b->poisoned = false;
    return 0;
}

// One call through the recorded graph: the bitstream is left at e->h_out + HX_ENC_GRAPH_OFF; returns false on failure.
static bool enc_graph_call(hx_enc *e, const float *pcm, int *nb, unsigned *frames)
{
    hx_batch *b = e->b;
    memcpy(e->h_pcm, pcm, (size_t) 1152 * b->nchan * sizeof(float));
    const volatile int *seq = reinterpret_cast<const volatile int *>(e->h_out) + 2;
    const int before = *seq;
    bool ok = hipGraphLaunch(e->gexec, e->gq) == hipSuccess;
    if (ok) {
        // wait on the sequence word the packing workgroup publishes behind its results (a few microseconds sooner than the
        // runtime's own wait); after 2 ms - a descheduled process, a contended device - leave the waiting to the runtime,
        // behind which the kernel's writes are complete as well
        const auto t0 = std::chrono::steady_clock::now();
        int spins = 0;
        while (*seq == before) {
            __builtin_ia32_pause();
            if ((++spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
        }
        if (*seq == before) ok = hipStreamSynchronize(e->gq) == hipSuccess;
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!ok) {
        (void) hipGetLastError();
        set_err("replaying the single-stream graph failed");
        b->poisoned = true;
        return false;
    }
    *nb = *reinterpret_cast<const volatile int *>(e->h_out);
    if (*nb < 0 || *nb > (int) e->outbuf.size()) *nb = 0;      // (cannot happen: the byte count is bounded by the stride)
    *frames = reinterpret_cast<const volatile unsigned *>(e->h_out)[1];
    return true;
}

// opt: the call's optional outputs (the packet of the *_Packet entry points; the encoder's batch has none set)
// packet_call: a *_Packet entry point's call, plain also where its packet argument is NULL (include/hmp3_amd.h)
static HX_IN_OUT encode_one(hx_enc *e, const float *pcm, unsigned char *bs_out, int in_bytes, const OptOut &opt = OptOut(), bool packet_call = false)
{
    HX_IN_OUT x = {in_bytes, 0};
    int nb = 0;
    unsigned frames = 0;
    const unsigned char *bs = nullptr;
    hx_batch *b = e->b;
    // The graph replays a call with exactly the arguments it was recorded with: anything optional (packets, debug taps)
    // goes the plain way, and so do the first two calls (which load the kernels).
    const bool plain = b->debug || opt.packet || packet_call || b->poisoned || b->inflight || e->graph_state < 0 || e->plain_calls < 2;
    if (!plain && e->graph_state == 0) {
        const char *env = getenv("HMP3AMD_ENC_GRAPH");
        const auto record = [&] { EncRecord alone(g_record_lock); return enc_graph_build(e); };
        if (env && atoi(env) == 0) e->graph_state = -1;
        else if (record() == 0) e->graph_state = 1;
        else {      // plain calls from here on (the staging stays allocated until the encoder is re-initialised or destroyed)
            if (e->gexec) { hipGraphExecDestroy(e->gexec); e->gexec = nullptr; }
            e->graph_state = -1;
        }
    }
    EncUse use(g_record_lock);
    if (!plain && e->graph_state == 1) {
        if (!enc_graph_call(e, pcm, &nb, &frames)) return x;
        bs = e->h_out + HX_ENC_GRAPH_OFF;
        e->graph_calls++;
    } else {
        // (encode_host's steps, with the call's own optional outputs in the record)
        const long long cap = (long long) e->outbuf.size();
        const auto pass = [&](Call c) { c.opt = opt; return encode_pass(b, {b->d_in, true}, 1, c, nullptr, PASS_PLAIN); };
        if (check_call(b, pcm, 1, e->outbuf.data(), cap, &nb) != 0 ||
            host_call(b, pcm, PcmIn{pcm, true}.bytes(1, 1, b->nchan), false, 1, e->outbuf.data(), cap, &nb, nullptr, pass) != 0) return x;
        bs = e->outbuf.data();
        frames = (unsigned) hx_batch_frames_bytes(b, 0).a;
        e->plain_calls++;
    }
    // a *_Packet call without a bitstream buffer: the frames count as sent, their bytes are neither returned nor counted
    // (mp3enc.cpp:2964-2994: bytesout = bs_out - bs_out0 stays 0)
    if (bs_out) memcpy(bs_out, bs, (size_t) nb);
    else nb = 0;
    x.out_bytes = nb;
    e->bytes += nb;
    e->ave = e->ave + ((((nb << 8) - e->ave)) >> (e->p.h_id ? 7 : 6));    // mp3enc.cpp:2328 / :2589
    e->frames = frames;
    return x;
}

extern "C" HX_IN_OUT hx_enc_L3_audio_encode(hx_enc *e, const float *pcm, unsigned char *bs_out)
{
    // float at int16 scale (pub/mp3enc.h:90-98), taken as is: the polyphase kernel reads fp32
    return encode_one(e, pcm, bs_out, 4608 * e->p.nchan);
}

// CMp3Enc::L3_audio_encode_Packet / MP3_audio_encode_Packet (pub/mp3enc.h:110-131): the normal
// bitstream in bs_out (may be NULL) plus this call's frame as a self-contained packet
// (nbytes_out[0] bytes, nbytes_out[1] = 0; at the MPEG-2 rates two packets, nbytes_out[0] then
// nbytes_out[1] bytes); packet may be NULL.
static HX_IN_OUT encode_packet(hx_enc *e, const void *pcm, int mp3_entry, unsigned char *bs_out, unsigned char *packet, int nbytes_out[2])
{
    OptOut opt;
    if (packet) {
        EncUse use(g_record_lock);
        hipSetDevice(e->device);
        if (!e->d_packet) { hipMalloc((void **) &e->d_packet, 4096); hipMalloc((void **) &e->d_packet_bytes, 2 * sizeof(int)); }
        opt.packet = e->d_packet; opt.packet_stride = 4096; opt.packet_bytes = e->d_packet_bytes;
    }
    float t[2304];      // (the MP3_audio_encode entry: convert, then encode)
    const int in_bytes = mp3_entry ? hx_src_convert(e->src, (const unsigned char *) pcm, t, nullptr) : 4608 * e->p.nchan;
    HX_IN_OUT x = encode_one(e, mp3_entry ? t : (const float *) pcm, bs_out, in_bytes, opt, true);
    if (packet) {
        EncUse use(g_record_lock);
        int n[2] = {0, 0};      // an MPEG-2 call returns two single-granule packets back to back (mp3enc.cpp:3363)
        hipMemcpy(n, e->d_packet_bytes, 2 * sizeof(int), hipMemcpyDeviceToHost);
        hipMemcpy(packet, e->d_packet, (size_t) (n[0] + n[1]), hipMemcpyDeviceToHost);
        nbytes_out[0] = n[0];
        nbytes_out[1] = n[1];
    }
    return x;
}

extern "C" HX_IN_OUT hx_enc_L3_audio_encode_Packet(hx_enc *e, const float *pcm, unsigned char *bs_out, unsigned char *packet, int nbytes_out[2])
{
    return encode_packet(e, pcm, 0, bs_out, packet, nbytes_out);
}

extern "C" HX_IN_OUT hx_enc_MP3_audio_encode_Packet(hx_enc *e, const unsigned char *pcm, unsigned char *bs_out, unsigned char *packet, int nbytes_out[2])
{
    return encode_packet(e, pcm, 1, bs_out, packet, nbytes_out);
}

static int nearest_rate(const int *table, int n, int x)
{
    int best = table[0], d0 = abs(table[0] - x);
    for (int i = 0; i < n; i++) { const int d = abs(table[i] - x); if (d < d0) { d0 = d; best = table[i]; } }
    return best;
}

// The encode control of a converted source: CMp3Enc::MP3_audio_encode_init's derivation (reference mp3enc.cpp:2655-2808),
// shared by hx_enc_MP3_audio_encode_init and the converting batches.  Picks the encode rate for the source rate and
// mpeg_select (0 track the input, 1 an MPEG-1 rate, 2 an MPEG-2 rate, else that rate), sets the converter `conv` up
// (hx_src.cpp) and writes the control the encoder behind it runs: the encode rate, mode 3 for a mono target, and
// nsb_limit bounded by the source's band when it is up-sampled.  Returns the bytes the caller must hold before every
// call (more than one call consumes: 1153 sample frames when the rates are equal), 0 on failure (hx_last_error).
int src_encode_control(const HX_E_CONTROL *ec, int source_bits, int source_is_float, int mpeg_select, int mono_convert,
                       hx_src *conv, HX_E_CONTROL *ec_out)
{
    static const int rate_table[6] = {22050, 24000, 16000, 44100, 48000, 32000};
    const int source = ec->samprate;
    if (source < 4000 || source > 48000) { set_err("source sample rate out of range"); return 0; }
    const int source_chan = (ec->mode == 3) ? 1 : 2;            // the source is mono iff ec->mode == 3
    const int target_chan = mono_convert ? 1 : source_chan;
    int target = 0;
    if (mpeg_select < 0) mpeg_select = 0;
    switch (mpeg_select) {
    case 0:
        if (source < 16000) { target = nearest_rate(rate_table, 3, 2 * source); if (target == 2 * source) break; }
        target = nearest_rate(rate_table, 6, source);
        break;
    case 1:
        if (source < 16000) { target = nearest_rate(rate_table + 3, 3, 4 * source); if (target == 4 * source) break; }
        if (source < 32000) { target = nearest_rate(rate_table + 3, 3, 2 * source); if (target == 2 * source) break; }
        target = nearest_rate(rate_table + 3, 3, source);
        break;
    case 2:
        if (source < 16000) { target = nearest_rate(rate_table, 3, 2 * source); if (target == 2 * source) break; }
        if (source > 24000) { target = nearest_rate(rate_table, 3, source / 2); if (2 * target == source) break; }
        target = nearest_rate(rate_table, 3, source);
        break;
    default:
        target = nearest_rate(rate_table, 6, mpeg_select);
        if (target != mpeg_select) { set_err("mpeg_select is not an MPEG sample rate"); return 0; }
        break;
    }
    int cutoff = 0;
    const int min_input_bytes = hx_src_init(conv, source, source_chan, source_bits, source_is_float, target, target_chan, &cutoff);
    if (min_input_bytes <= 0) { set_err("the sample-rate converter cannot handle this source format / rate pair"); return 0; }
    int nsb_limit = (64 * cutoff + target / 2) / target;
    if (nsb_limit > 30) nsb_limit = 30;
    HX_E_CONTROL ec2 = *ec;
    ec2.samprate = target;
    if (target_chan == 1) ec2.mode = 3;
    if (source < target) {          // up-sampled input has nothing above the source's band
        if (ec2.nsb_limit <= 0) ec2.nsb_limit = 30;
        if (ec2.nsb_limit > nsb_limit) ec2.nsb_limit = nsb_limit;
    }
    ec2.layer = 3;
    *ec_out = ec2;
    return min_input_bytes;
}

extern "C" int hx_src_encode_control(const HX_E_CONTROL *ec, const HX_SOURCE *src, HX_E_CONTROL *ec_out)
{
    if (!ec || !src || !ec_out) { set_err("bad arguments"); return 0; }
    hx_src *conv = hx_src_create();
    const int r = src_encode_control(ec, src->bits, src->is_float, src->mpeg_select, src->mono_convert, conv, ec_out);
    hx_src_destroy(conv);
    return r;
}

// CMp3Enc::MP3_audio_encode_init (reference mp3enc.cpp:2655-2808): the converter and the encoder behind it (see
// src_encode_control).  Returns the bytes the caller must hold before every hx_enc_MP3_audio_encode call, 0 on failure.
extern "C" int hx_enc_MP3_audio_encode_init(hx_enc *e, const HX_E_CONTROL *ec, int source_bits, int source_is_float,
                                            int mpeg_select, int mono_convert)
{
    if (!e->src) e->src = hx_src_create();
    HX_E_CONTROL ec2;
    const int min_input_bytes = src_encode_control(ec, source_bits, source_is_float, mpeg_select, mono_convert, e->src, &ec2);
    if (!min_input_bytes) return 0;
    if (!hx_enc_L3_audio_encode_init(e, &ec2)) return 0;
    e->src_bits = source_bits;
    e->src_float = source_is_float;
    e->src_chan = (ec->mode == 3) ? 1 : 2;
    return min_input_bytes;
}

// CMp3Enc::MP3_audio_encode (mp3enc.cpp:2812-2828): convert, then encode; in_bytes is what the converter used.
// pcm must hold the bytes hx_enc_MP3_audio_encode_init returned, and be readable for
// 1152 * (source rate / encode rate + 1) sample frames (the converter stages that many).
extern "C" HX_IN_OUT hx_enc_MP3_audio_encode(hx_enc *e, const unsigned char *pcm, unsigned char *bs_out)
{
    float t[2304];
    return encode_one(e, t, bs_out, hx_src_convert(e->src, pcm, t, nullptr));
}

extern "C" void hx_enc_out_stats(hx_enc *e)
{
    int calls = 0;
    if (e && e->b) {
        EncUse use(g_record_lock);
        hipSetDevice(e->b->device);
        hipDeviceSynchronize();
        hipMemcpy(&calls, (char *) e->b->d_st + offsetof(HxStream, call_count), sizeof(int), hipMemcpyDeviceToHost);
    }
    fprintf(stderr, "\n ba long  %6d %6d %6d %6d %6d %6d %6d %6d %6d", calls, 0, 0, 0, 0, 0, 0, 0, 0);
}

// Which route the calls since init took (include/hmp3_amd.h, "test taps"): plain calls, replayed calls, graph_state.
extern "C" int hx_enc_debug_calls(hx_enc *e, int out[3])
{
    if (!e || !out) return -1;
    out[0] = e->plain_calls;
    out[1] = e->graph_calls;
    out[2] = e->graph_state;
    return 0;
}

extern "C" unsigned hx_enc_get_frames(hx_enc *e) { return e->frames; }
extern "C" HX_INT_PAIR hx_enc_get_frames_bytes(hx_enc *e) { HX_INT_PAIR r = {(int) e->frames, (int) e->bytes}; return r; }
extern "C" float hx_enc_get_bitrate_float(hx_enc *e)
{
    if (e->frames <= 0) return 0.0f;
    const float samples = e->p.h_id ? 1152.0f : 576.0f;        // per frame: MPEG-1 / MPEG-2 (mp3enc.cpp:3456-3462)
    return ((0.001f * 8.0f) * e->bytes * e->p.samprate / (samples * e->frames));
}
extern "C" int hx_enc_get_bitrate(hx_enc *e) { return (int) (hx_enc_get_bitrate_float(e) + 0.5f); }
extern "C" float hx_enc_get_bitrate2_float(hx_enc *e)
{
    if (e->frames <= 0) return 0.0f;
    return (float) ((0.001f * 8.0f / (1152.0 * 256.0)) * e->ave * e->p.samprate);
}
extern "C" void hx_enc_info_ec(hx_enc *e, HX_E_CONTROL *ec) { memcpy(ec, &e->p.ec, sizeof(HxControl)); }
extern "C" void hx_enc_info_head(hx_enc *e, HX_MPEG_HEAD *h) { memcpy(h, &e->p.head_info, sizeof(HxMpegHead)); }
extern "C" void hx_enc_info_string(hx_enc *e, char *s)
{
    static const char *mode_msg[4] = {"stereo", "joint stereo", "dual", "mono"};
    const HxControl *ec = &e->p.ec;
    s += sprintf(s, "Layer III   %s ", mode_msg[e->p.h_mode & 3]);
    s += sprintf(s, "  %ldHz ", (long) e->p.samprate);
    if (ec->vbr_flag == 0) s += sprintf(s, "  %dkbps ", e->p.totbitrate);
    else {
        s += sprintf(s, " VBR-%d", ec->vbr_mnr);
        if (ec->vbr_delta_mnr) s += sprintf(s, "(%d)", ec->vbr_delta_mnr);
    }
    if (ec->hf_flag) { s += sprintf(s, "  hf"); if (ec->hf_flag & 2) s += sprintf(s, "2"); }
}
