// hx_rt.h - what the units of the host runtime share: the batch, its error / allocation helpers, the kernels' prototypes
// and the few entry points one unit needs of another.  Units: hx_batch.hip (the batch and its passes), hx_batch_src.hip
// (converting batches), hx_batch_slots.hip (slot state: reset, save, restore), hx_enc.cpp (the single-stream encoder),
// hx_multi.cpp (several devices behind one handle).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
#include <hip/hip_runtime_api.h>    // (a unit that launches no kernel is built by the host compiler)
#endif
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <vector>
#include <algorithm>
#include "../../include/hmp3_amd.h"
#include "hx_types.h"
#include "hx_host.h"
#include "hx_src.h"

// what one unit of the library needs of another is not an export
#define HX_LOCAL __attribute__((visibility("hidden")))

HX_LOCAL void set_err(const char *fmt, const char *a = "");       // the calling thread's hx_last_error
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err("HIP error: %s", hipGetErrorString(e_)); return -1; } } while (0)
#define HIPCHKN(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err("HIP error: %s", hipGetErrorString(e_)); return nullptr; } } while (0)

#ifdef __HIPCC__
// kernels (hx_polyphase.hip / hx_spec.hip / hx_prep.hip / hx_alloc.hip / hx_pack.hip with hx_crc.hip, hx_slots.hip, hx_ledger.hip, hx_pcmin.hip and hx_fileimg.hip / hx_src.hip)
// (K1_GPB / K1_THREADS, k_polyphase's tile and launch dimension: hx_types.h)
// nfr (the last argument of every kernel that walks a stream's granules or frames; AllocArgs::nfr for the stream walk): [S] the
// frames each stream takes of the call (hx_batch_frame_counts), or null = all of them.  A kernel bounds its work on stream s
// by 2 * nfr[s] granules; NG, nsamp and frames_per_stream stay the strides of the rows.
// pitch (the kernels that read PCM): the channels every PCM row is laid out for, hx_batch::nchan; a stream's own channel
// count comes from its class (HxParams::nchan) or its plan (HxSrcPlan::nch).
__global__ void k_polyphase(const int16_t *pcm, long long nsamp, const HxStream *st, const HxParams *prm,
                            const HxGlobalTabs *gt, float *sb, int NG, int SG, const float *pcmf, int pitch, int *eng, const int *nfr);
__global__ void k_dcfilter(const int16_t *pcm, const float *pcm32, long long nsamp, HxStream *st, const HxParams *prm, float *pcmf, int S, int pitch, const int *nfr);
__global__ void k_src(SrcArgs a);
__global__ void k_detect(HxStream *st, const HxParams *prm, const int *eng, unsigned char *flg, int *dbg_metric, unsigned char *bt,
                         unsigned char *btprev, int NG, int S, const int *nfr);
__global__ void k_spec(const float *sb, const HxStream *st, const HxParams *prm, const HxGlobalTabs *gt, const unsigned char *bt,
                       float *xr, float *etab, float *thr, int *msbase, int NG, int SG, const int *nfr);
__global__ void k_spec_direct(const float *sb, const HxStream *st, const HxParams *prm, const HxGlobalTabs *gt, const unsigned char *bt,
                              float *xr, float *etab, float *thr, int *msbase, int NG, int SG, const int *nfr);
__global__ void k_msscan(HxStream *st, const HxParams *prm, const int *msbase, const unsigned char *bt, unsigned char *msflag, int *msdec,
                         const float *thr, float *thrprev, int NG, float *sb, int SG, const int16_t *pcm, long long nsamp, const float *pcmf, int pitch, const int *nfr);
__global__ void k_prep(const float *xr, float *xmag_dbg, float *x34o, unsigned *sgn, HxBandPrep *band, const HxStream *st, const HxParams *prm, const HxGlobalTabs *gt,
                       const unsigned char *bt, const unsigned char *msflag, const float *etab, const float *thr, const float *thrprev, int NG, long long nunits, const int *nfr);
__global__ void k_pack(const HxStream *st, const HxParams *prm, const HxGlobalTabs *gt, const short *ixq, const unsigned *sgn, const HxSegOut *seg,
                       const HxFrameOut *frm, const HxSlot *slots, unsigned char *out, long long out_stride, unsigned char *packet, int *status,
                       int frames_per_stream, int NG, long long nframes_total, int solo, HxStream *st_w, const int *pre_len, const int *out_bytes,
                       const int *carry_len, unsigned *frames_out, unsigned char *host_out, const int *seq_src, const int *nfr);
__global__ void k_pack_carry(HxStream *st, const unsigned char *out, long long out_stride, const int *out_bytes, const int *carry_len, unsigned *frames_out);
__global__ void k_pack_pre(const HxStream *st, unsigned char *out, long long out_stride, const int *pre_len);
__global__ void k_dense_off(const int *out_bytes, long long *off, long long *off_copy, int S, long long cap, int *status);
__global__ void k_dense_gather(const unsigned char *out, long long out_stride, const int *out_bytes, const long long *off, unsigned char *dense,
                               long long cap, int chunks);
__global__ void k_crc(const unsigned char *out, long long out_stride, const int *out_bytes, const int *stats, int nframes, unsigned short *crc);
__global__ void k_recon_hybrid(const HxStream *st, const HxParams *prm, const HxGlobalTabs *gt, const HxReconTabs *rt, const short *ixq, const unsigned *sgn,
                               const HxSegOut *seg, const HxFrameDebug *rec, float *hyb, float *tails, const float *state, int NG, const int *nfr);
__global__ void k_recon_synth(const HxStream *st, const HxParams *prm, const HxReconTabs *rt, const float *hyb, const float *state, float *out,
                              long long row, int NG, const int *nfr);
__global__ void k_recon_carry(const HxStream *st, const HxParams *prm, const float *hyb, const float *tails, float *state, int NG, const int *nfr);
__global__ void k_slot_reset(SlotArgs a);
__global__ void k_slot_gather(SlotArgs a, uint2 *blobs);
__global__ void k_slot_scatter(SlotArgs a, const uint2 *blobs);
__global__ void k_ledger(HX_LEDGER *led, const int *stats, const unsigned short *crc, const int *out_bytes, const int *nfr, int nframes, int S);
__global__ void k_ledger_begin(HX_LEDGER *led, const HxLedgerEntry *ent);
__global__ void k_ledger_gather(const HX_LEDGER *led, const HxLedgerEntry *ent, HX_LEDGER *out);
__global__ void k_pcm_spread(const unsigned char *img, const long long *off, unsigned char *rows, long long row_bytes, int nframes, int sample_bytes,
                             const HxStream *st, const HxParams *prm, const int *nfr, int chunks);
__global__ void k_pcm_planes(const unsigned char *img, const long long *pl, int S, unsigned char *rows, long long row_bytes, int nframes, int sample_bytes,
                             int unit, const HxStream *st, const HxParams *prm, const int *nfr, int chunks);
__global__ void k_file_append(const HX_LEDGER *led, uint2 *fw, unsigned char *img, long long pitch, long long cap, const unsigned char *out, long long out_stride,
                              const int *nfr, int nframes, int chunks, int *status);
__global__ void k_file_begin(uint2 *fw, const HxLedgerEntry *ent, int n, unsigned on);
__global__ void k_ledger_brief(const HX_LEDGER *led, const uint2 *fw, HX_LEDGER_BRIEF *out, int S);
__global__ void k_file_tag(const HX_LEDGER *led, const uint2 *fw, unsigned char *img, long long pitch, long long cap, const HxFileTagEntry *ent);
__global__ void k_file_off(const HxLedgerEntry *ent, int n, const HX_LEDGER *led, const uint2 *fw, long long cap, long long *off, long long dst_cap, int *status);
__global__ void k_file_gather(const HxLedgerEntry *ent, const HX_LEDGER *led, const uint2 *fw, const unsigned char *img, long long pitch, long long cap,
                              const long long *off, unsigned char *dst, long long dst_cap, int chunks);
__global__ void k_order(const unsigned *dur, int *order, int S);
__global__ void k_order_kinds(const unsigned *dur, const HxStream *st, const HxParams *prm, int *order, int S);
__global__ void k_gate(const unsigned *done_counter, unsigned base, unsigned need, int *timeouts);
__global__ void k_alloc(AllocArgs a);
__global__ void k_alloc_slim(AllocArgs a);
__global__ void k_alloc_lsf(AllocArgs a);
__global__ void k_alloc1(AllocArgs a);
__global__ void k_alloc1_lsf(AllocArgs a);
__global__ void k_debug_count(AllocArgs a, HxCountArgs c);          // (hx_alloc3.inc, one per stream-walk unit: the units' twins hx_count*.hip)
__global__ void k_debug_count_slim(AllocArgs a, HxCountArgs c);
__global__ void k_debug_count_lsf(AllocArgs a, HxCountArgs c);
__global__ void k_debug_count_a1(AllocArgs a, HxCountArgs c);
__global__ void k_debug_count_a1_lsf(AllocArgs a, HxCountArgs c);
__global__ void k_debug_math(int fn, const unsigned *in, long long n, unsigned *out, const HxGlobalTabs *gt, const HxParams *gp);     // (hx_alloc1.inc, the k_alloc1 unit)

// every kernel launch is checked where it is made: a bad configuration or a lost device is reported
// with the kernel's name instead of surfacing at some later call
#define LAUNCH_LDS(kernel, grid, block, lds, stream, ...) do { hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__); \
        hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { set_err("launch of " #kernel " failed: %s", hipGetErrorString(e_)); return -1; } } while (0)
#define LAUNCH(kernel, grid, block, stream, ...) LAUNCH_LDS(kernel, grid, block, 0, stream, __VA_ARGS__)
#endif

// The buffers that hand a call's granules from the front end to the stream walk (layouts: AllocArgs).
// The submit path keeps two sets: the front end of call n + 1 fills one while the stream walk of call n reads the other.
struct FrontSet {
    float *xr, *etab, *thr;
    float *x34;                         // x^(3/4) of the magnitudes (k_prep writes it in debug mode only)
    float *thrprev;                     // [S][2][64] pre-echo memory at the call's start
    int *msbase, *msdec;
    unsigned char *bt, *btprev, *msflag;
    HxBandPrep *band;
};
// ... and from the stream walk to the packing: quantised lines, segment and frame records, slot lists, and the byte counts of
// the pending frames' images at the call's start / end (views into hx_batch::d_lens)
struct WalkSet {
    short *ixq;
    HxSegOut *seg;
    HxFrameOut *frm;
    HxSlot *slots;
    int *pre_len, *carry_len;
    HxFrameDebug *rec;                  // [S][maxF] the set's own frame records, which the decoded-PCM kernels read (made when
                                        // hx_batch_recon_buffer is first switched on, null before)
};

// Where a call's dense image goes (hx_batch_dense_buffers): buf null = off.  off_copy: a second place for the offsets (the
// pipelined host calls, whose offsets go to the caller's page-locked array as well as to device staging).
struct DenseOut { unsigned char *buf = nullptr; long long cap = 0; long long *off = nullptr, *off_copy = nullptr; };
// The optional outputs of a call, all in device memory, null = off: every frame as a packet (hx_batch_packet_buffers), the
// per-frame counters (hx_batch_frame_stats_buffer), the dense image and the per-frame MusicCRC (hx_batch_crc_buffer; k_crc
// reads the counters, so a call with crc needs frame_stats: check_opt) and the decoded PCM (hx_batch_recon_buffer).
struct OptOut { unsigned char *packet = nullptr; long long packet_stride = 0; int *packet_bytes = nullptr, *frame_stats = nullptr; DenseOut dense; unsigned short *crc = nullptr;
                float *recon = nullptr; };
// The file images of a batch (hx_batch_file_images): img null = off.  [S] images of `pitch` bytes each, of which `cap` count;
// fw [S][2]: per slot {image_bytes, the record has an image} (hx_fileimg.hip) - made at the first switch-on and kept
struct FileImages { unsigned char *img = nullptr; long long pitch = 0, cap = 0; unsigned *fw = nullptr; };
// Everything one call writes, fixed when the call is made: the rows, the optional outputs and, for the pass the one-stream
// encoder records into a HIP graph (hx_enc.cpp; no timing events, nothing that queries the stream), where k_pack_carry
// leaves the stream's frame counter and the page-locked host memory the packing workgroup publishes the call's results to
// (hx_pack.hip).  The stream walk and the packing get this record, so nothing set on the batch afterwards reaches the call.
struct Call {
    unsigned char *out = nullptr; long long out_stride = 0; int *out_bytes = nullptr;
    OptOut opt;
    const int *nfr = nullptr;           // device copy of the per-stream frame counts in force when the call was made (encode_pass
                                        // uploads it: hx_batch::nfr_stage; a converting call under counts has, in front of k_src),
                                        // null = every stream takes the call's nframes
    unsigned *rec_frames = nullptr; unsigned char *rec_host = nullptr; bool recording = false;
    HX_LEDGER *ledger = nullptr;        // the batch's file ledger as it stood when the call was made (null: none yet): k_ledger goes out behind the call's k_crc
    FileImages files;                   // ... and its file images (img null: off): k_file_append goes out behind the call's k_ledger
};

// Three staging copies in rotation for a small list that a call hands to its kernels: page-locked host memory and device
// memory, [3][bytes] each, and one event per copy that says when the copy's last user is done (operations below, behind
// dev_alloc).  Which copy a call takes, and behind what it records the event, is the call's own business.
struct Staging {
    char *h = nullptr, *d = nullptr;
    size_t bytes = 0;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};     // (a never-recorded event counts as done)
    template <class T> T *dev(int k) const { return (T *) (d + (size_t) k * bytes); }
};

struct hx_batch {
    int device = 0, S = 0, maxF = 0, ncls = 0;
    std::vector<HxParams> params;       // host copy per class
    std::vector<int> cls_of;            // stream -> class
    // The menu of configurations the batch was created with (hx_batch_create_menu; hx_batch_create[_src]: their deduplicated
    // controls): entry -> class and (converting batches) entry -> plan, identical entries sharing theirs, and the caller's
    // entry each slot runs.  cfg_of, cls_of and src_cls move when hx_batch_assign_streams is called; the device follows in
    // stream order.
    std::vector<int> menu_cls, menu_plan, cfg_of;
    HxParams *d_prm = nullptr;
    HxGlobalTabs *d_gt = nullptr;
    HxStream *d_st = nullptr;
    float *d_sb = nullptr, *d_xrdbg = nullptr;
    FrontSet front[2] = {};             // [1]: created at the first submit (pipe_init)
    WalkSet walk[2] = {};
    unsigned *sgn[3] = {};              // the lines' signs, one bit per line: [S][NG][2][HX_SGN_WORDS]; read by the packing, so three sets
                                        // on the submit path (the front end of call n + 2 writes one while call n is packed)
    int *d_lens = nullptr;              // [2 sets][pre_len | carry_len][S]
    OptOut opt;                         // the caller's optional outputs: what the three setters leave, and what a call made now takes (call_on)
    float *d_pcmf = nullptr;            // DC-blocked input, only when a stream uses filter_select = 1
    bool any_dc = false;
    int nchan = 2;                      // P, the pitch: channels every PCM row (the caller's, d_pcmf, d_src_pcm) is laid out for = the largest
                                        // over the menu.  A stream's own count is its class's (params[cls].nchan): they differ in a mixed batch only
    // A class's kind = 2 * alloc1 + lsf: alloc1 = the first-generation allocator (intensity stereo, dual channel), lsf = an
    // MPEG-2 rate (16 / 22.05 / 24 kHz), where every 1152-sample block yields two frames.  Each kind has its own stream-walk
    // kernel.  kinds: the kinds of the menu's classes as a bit mask; a batch of one kind (every create call but
    // hx_batch_create_any allows no other) has that kind in lsf / alloc1 and walks all streams in one launch.  With several
    // kinds, lsf = 1 when any class is MPEG-2 (the frame positions per block the packing covers: AllocArgs::fpc) and alloc1
    // is not used: launch_walk makes one launch per kind over its span of the order k_order_kinds made.
    int lsf = 0, alloc1 = 0;
    unsigned kinds = 0;
    std::vector<int> cls_kind;          // class -> kind
    int slim = 0;                       // 1: the low-footprint stream walk k_alloc_slim (six streams per CU instead of four) for the kind-0 streams, chosen at create
    int *d_eng = nullptr, *d_status = nullptr, *d_dbgmetric = nullptr;
    unsigned char *d_flg = nullptr;
    HxFrameDebug *d_dbg = nullptr;
    unsigned long long *d_prof = nullptr;
    int lastNG = 0;                     // NG of the previous call (the debug taps' row stride)
    // per-stream frame counts (hx_batch_frame_counts; of a converting batch the counts of the hx_batch_encode_src_counts_*
    // call being made, empty between calls): the host copy a call checks and takes (empty = uniform calls) and its
    // staging, [S] counts per copy, in rotation with the sets of signs - a device-buffer submit's deferred packing still
    // reads its copy while two later submits are in flight.  A copy's event: the upload out of it is done.
    std::vector<int> nfr;
    Staging nfr_stage;
    long long nplain = 0;               // plain calls made under counts (they rotate the copies too: no call waits for its predecessor's upload)
    // PCM segments (hx_batch_pcm_segments): the host copy a call checks and takes - seg_off [S] byte offsets into the call's
    // image of seg_bytes bytes, empty = rows - and its staging, [S] offsets per copy, in the rotation of the counts' (a
    // submit: the copy of its set of signs; plain calls: their own count, nplain_img).  d_rows: the row buffer k_pcm_spread
    // fills and the front end reads in place of the caller's pointer, [S][nframes * 1152 * P] samples of the call's type; one
    // for all pass kinds (the front end's stream is in order), made at the first call under segments and grown behind a
    // drain.  rows_bytes: what the last call under segments or planes used of it (the "pcmrows" tap).
    // PCM planes (hx_batch_pcm_planes) exclude segments and share all of this but the host copy: pl_off [S] the byte offsets of
    // the streams' plane 0 in the image of pl_bytes bytes (empty = not in force), pl_stride [S] the byte distance from a
    // stream's plane 0 to its plane 1 (empty = tight, the plane's own length as of the call), pl_unit: fp32 samples are at
    // unit scale.  img_stage is sized for the planes' layout (planes_stage_bytes); a call under segments sends the first
    // segs_stage_bytes of its copy.
    std::vector<long long> seg_off;
    long long seg_bytes = 0;
    std::vector<long long> pl_off, pl_stride;
    long long pl_bytes = 0;
    bool pl_unit = false;
    Staging img_stage;
    long long nplain_img = 0;
    unsigned char *d_rows = nullptr; long long rows_cap = 0, rows_bytes = 0;
    // converting batches (hx_batch_create_src): k_src turns each stream's source into the fp32 PCM the front end reads
    int nsrc = 0;                       // converter plans, deduplicated (0: not a converting batch)
    std::vector<HxSrcPlan> src_plans;
    std::vector<int> src_cls;           // stream -> plan
    std::vector<long long> src_calls;   // stream -> converter calls made (authoritative; the device keeps a copy for k_src)
    HxSrcPlan *d_src_plan = nullptr;
    int *d_src_cls = nullptr;
    long long *d_src_calls = nullptr;   // [2][S]: k_src reads copy src_par and writes the other
    float *d_src_carry = nullptr;       // [2][S][2][HX_SRC_CARRY] the same for the case-4 intermediate samples
    int src_par = 0;
    float *d_src_pcm = nullptr;         // [S][nframes * 1152 * nchan] the last call's converted PCM, laid out like a plain call's
    long long *d_src_off = nullptr, *h_src_off = nullptr;      // [S][max_frames] the caller's frame offsets (device / page-locked)
    hipEvent_t ev_src_off = nullptr;    // the last upload of h_src_off is done
    int src_xwin = 0, src_zwin = 0, src_zoff = 0, src_coff = 0, src_lastF = 0;
    size_t src_lds = 0;
    // slot operations (hx_batch_reset_streams, hx_batch_get / set_stream_states*): what a new stream of each class starts with
    // and each class's blob fingerprint (made at create), of a converting batch each stream's plan fingerprint; the entry lists'
    // staging, [S] HxSlotEntry per copy (made at the first operation) - the host refills copy k when the operation three
    // before, upload and kernel, is done; the host-blob calls' device staging
    HxStream *d_init = nullptr;         // [ncls]
    std::vector<unsigned long long> cls_fp;     // [ncls]
    unsigned long long *d_src_fp = nullptr;     // [S]
    unsigned long long *d_plan_fp = nullptr;    // [nsrc] each plan's fingerprint (k_slot_reset takes a slot's from here)
    Staging ent_stage;
    long long nslotops = 0;
    std::vector<long long> slot_mark;   // [S] the last operation that listed the slot (duplicates)
    long long slot_serial = 0;
    unsigned char *d_blobs = nullptr; long long blobs_cap = 0;
    // the file ledger (hx_batch_ledger_*): [S] records, made and zeroed at the first hx_batch_ledger_begin, and which of them
    // the host takes for live - begun, and not shown ended by a hx_batch_ledger_read since (a call that feeds a live record
    // needs frame counters and CRCs: check_opt)
    HX_LEDGER *d_ledger = nullptr;
    std::vector<unsigned char> led_live;
    // file images (hx_batch_file_images): the images and the length words, and the host's view of each slot's head_bytes
    // (its latest hx_batch_ledger_begin's; it moves when that call is made, like led_live)
    FileImages files;
    std::vector<int> led_head;
    // finished files (hx_batch_file_tags, hx_batch_file_fetch_many): which slots' latest begin was made with images on (like
    // led_head); the tag entries' staging, [S] HxFileTagEntry per copy, made at the first hx_batch_file_tags, in the slot
    // operations' rotation (nslotops); the host fetch's device staging - the dense image, grown to the largest total so far and
    // released with the images, and its offsets [S + 1] - and the list of the scan that the gather behind it reads
    std::vector<unsigned char> led_img;
    Staging tag_stage;
    unsigned char *d_many = nullptr; long long many_cap = 0;
    long long *d_many_off = nullptr;
    int many_k = 0;
    bool debug = false;
    // decoded PCM (hx_batch_recon_buffer), all made at the first switch-on (recon_reserve) and kept: the kernels' tables, the
    // streams' carried state [S][HX_RECON_STATE_FLOATS] (outside HxStream and the checkpoint blob), the hybrid output of the
    // call being reconstructed [S][2 maxF][2][576] and its last tails [S][2][576] - one of each: the decoded-PCM kernels of
    // consecutive calls run one after the other, behind their packing, which is ordered the same way by the frames it carries
    HxReconTabs *d_recon_tabs = nullptr;
    float *d_recon_state = nullptr, *d_recon_hyb = nullptr, *d_recon_tails = nullptr;
    float *d_reconh = nullptr; long long reconh_cap = 0;        // the *_host_recon calls' device staging
    // staging for the host-buffer entry points (host_call): the caller's input as it came (PCM, or a converting batch's
    // source bytes), the bitstream, its byte counts and the per-frame counters of the calls that return them
    void *d_in = nullptr; unsigned char *d_out = nullptr; int *d_outbytes = nullptr, *d_stats = nullptr;
    long long in_cap = 0, out_cap = 0, stats_cap = 0;
    unsigned char *d_dense = nullptr; long long *d_dense_off = nullptr; long long dense_cap = 0;   // ... and of the *_host_dense calls: image and offsets
    unsigned short *d_crc = nullptr; long long crc_cap = 0;                                         // ... and of the *_host_crc calls: the per-frame CRCs
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double alloc_ms_sum = 0; int alloc_calls = 0;
    // hx_batch_submit_*: the front-end kernels of call n+1 run (low-priority stream) while k_alloc of
    // call n (high-priority stream) works through its slowest streams (see FrontSet)
    hipStream_t s_front = nullptr, s_alloc = nullptr, s_pack = nullptr;
    hipEvent_t ev_in = nullptr, ev_front[2] = {nullptr, nullptr}, ev_alloc[2] = {nullptr, nullptr};     // ev_alloc: a submit's packing is done (everything is)
    hipEvent_t ev_k6[2] = {nullptr, nullptr};           // a submit's allocator launch is done
    hipEvent_t ev_sgn[3] = {nullptr, nullptr, nullptr}; // the packing that read this set of signs is done
    // the packing of the latest device-buffer submit, not enqueued yet: it goes out behind the next submit's allocator launch
    // (released by a gate like the front end, into that launch's tail), or ungated at the next wait / plain call
    // (call: the submit's record - the stream walk has put the packets' headers into its packet buffer already, and the image
    // kernels go out with the packing)
    struct PackJob { bool pending = false; Call call; int nframes = 0, set = 0, sset = 0; } pack_job;
    long long nsubmit = 0;
    bool inflight = false;
    // hx_batch_submit_*_host: device staging for two calls in flight and the copy streams
    void *hs_pcm[2] = {nullptr, nullptr}; unsigned char *hs_out[2] = {nullptr, nullptr}; int *hs_nb[2] = {nullptr, nullptr};
    long long *hs_off[2] = {nullptr, nullptr};      // the dense submits' offsets (the gather reads them here, not over the link)
    long long hs_pcm_cap = 0, hs_out_cap = 0;
    hipStream_t s_h2d = nullptr, s_d2h = nullptr, s_host = nullptr;
    hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_d2h[2] = {nullptr, nullptr}, ev_hfront[2] = {nullptr, nullptr};
    long long nhost = 0;
    unsigned *d_dur = nullptr;          // [S] duration of each stream's allocator workgroup in the last launch
    int *d_order = nullptr;             // [S] workgroup -> stream for the next launch (used when the batch exceeds what the chip holds at once)
    int *d_done = nullptr;              // [HX_CNT_WORDS] the counter block (hx_types.h, HxCounter)
    int resident = 0;                   // allocator workgroups the device holds at once
    long long alloc_launches = 0;
    unsigned long long cfg_hash = 0;    // fingerprint of the resolved configuration classes (checkpoint blobs carry their stream's)
    // a submit's front end is released once this share of the previous allocator launch's resident set has started.
    // Not 100: the gate's own wavefront holds register space on one SIMD, so the last allocator workgroup of a full
    // chip cannot start before a stream retires (measured: 10 .. 99 % all give the same step time, 100 % loses 30 %)
    int gate_percent = 90;
    bool poisoned = false;              // a HIP call failed in the middle of a pass: the event bookkeeping is incomplete, further calls are refused
    // longest-first workgroup order: 2 = for every batch with more streams than the chip has CUs (default: below that no two
    // streams share a CU and the order decides nothing), 3 = always (tests), 1 = only for batches beyond the resident set,
    // 0 = never (HMP3AMD_LPT).
    // Beyond the resident set it keeps the launch's last round short.  Within it the order decides which streams share a CU:
    // workgroups are dealt over XCDs and CUs in turn, so a CU's four streams are 256 apart in launch order - in stream order
    // those are streams of one residue class, and a batch whose slow streams recur with a period (BASELINE config 5: correlation
    // by stream mod 4) had them all on the same CUs; sorted by the previous call's duration a CU gets one stream of each quartile.
    // (Round 4: config 2 +1.0 %, its worst-case signal set +2.1 %.)
    int lpt = 2;
    int ncu = 256;                      // compute units of the device
    int park_k = 8;                     // HMP3AMD_PARK: the CUs of this many longest streams are kept free of other kernels' workgroups (0 = off; see hx_alloc3.inc, "parking")
    int park_pair = 0;                  // HMP3AMD_PARK_PAIR=1: also the CU that shares the instruction cache with a straggler's
    int strict_sums = 0;                // HMP3AMD_EXACT_SUMS=1: the stream walk adds every band in line order instead of certifying a parallel sum (tests)
    // everything the batch allocates or creates on the device (dev_alloc, new_stream, new_event) and its page-locked host
    // memory (host_alloc): hx_batch_destroy releases it
    std::vector<void *> mem, pinned;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> events;
};

// more than one kind of stream in the menu (hx_batch_create_any): one stream-walk launch per kind
static inline bool several_kinds(const hx_batch *b) { return (b->kinds & (b->kinds - 1)) != 0; }
// frames per 1152-sample block of a class: 1, or 2 at the MPEG-2 rates
static inline int frames_per_block(const HxParams &p) { return p.h_id ? 1 : 2; }

// Every device buffer, HIP stream and event of a batch is made by one of these and listed in the batch, whose
// hx_batch_destroy releases them.
template <class T> static int dev_alloc(hx_batch *b, T *&p, long long bytes)
{
    void *q = nullptr;
    if (hipMalloc(&q, (size_t) bytes) != hipSuccess) { set_err("hipMalloc failed"); return -1; }
    b->mem.push_back(q);
    p = (T *) q;
    return 0;
}
// (staging that grows with the call: the old buffer is freed, its contents are not kept)
template <class T> static int dev_realloc(hx_batch *b, T *&p, long long bytes)
{
    if (p) {
        hipFree(p);
        for (void *&m : b->mem) if (m == p) { m = b->mem.back(); b->mem.pop_back(); break; }
        p = nullptr;
    }
    return dev_alloc(b, p, bytes);
}
// ... to at least `bytes`, where cap is what it holds
template <class T> static int dev_grow(hx_batch *b, T *&p, long long &cap, long long bytes)
{
    if (bytes <= cap) return 0;
    if (dev_realloc(b, p, bytes) != 0) return -1;
    cap = bytes;
    return 0;
}
template <class T> static int host_alloc(hx_batch *b, T *&p, size_t bytes)
{
    void *q = nullptr;
    if (hipHostMalloc(&q, bytes, 0) != hipSuccess) { set_err("hipHostMalloc failed"); return -1; }
    b->pinned.push_back(q);
    p = (T *) q;
    return 0;
}
HX_LOCAL int new_stream(hx_batch *b, hipStream_t &q, int priority = INT_MAX);     // (INT_MAX: the runtime's default priority)
HX_LOCAL int new_event(hx_batch *b, hipEvent_t &e);

// A Staging's four operations.  make: its pieces, `bytes` per copy, each made once - a call that fails half way leaves what
// it made to the next one (and to hx_batch_destroy), which makes only the rest.  take: wait on the host until copy k's event
// is done and hand out its host memory to fill (null: the wait failed).  upload: the first n bytes of copy k to the device
// on stream q.  done: copy k's event on stream q.
static inline int staging_make(hx_batch *b, Staging &s, size_t bytes)
{
    s.bytes = bytes;
    if (!s.h && host_alloc(b, s.h, 3 * bytes) != 0) return -1;
    for (int k = 0; k < 3; k++)
        if (!s.ev[k] && new_event(b, s.ev[k]) != 0) return -1;
    return s.d ? 0 : dev_alloc(b, s.d, (long long) (3 * bytes));
}
static inline void *staging_take(Staging &s, int k)
{
    const hipError_t e = hipEventSynchronize(s.ev[k]);
    if (e != hipSuccess) { set_err("HIP error: %s", hipGetErrorString(e)); return nullptr; }
    return s.h + (size_t) k * s.bytes;
}
static inline int staging_upload(Staging &s, int k, size_t n, hipStream_t q)
{
    HIPCHK(hipMemcpyAsync(s.dev<char>(k), s.h + (size_t) k * s.bytes, n, hipMemcpyHostToDevice, q));
    return 0;
}
static inline int staging_done(Staging &s, int k, hipStream_t q) { HIPCHK(hipEventRecord(s.ev[k], q)); return 0; }

// A launch or HIP call that fails once a pass has touched the batch leaves events unrecorded, buffer sets half handed
// over or staging half updated: the batch is not reusable (this only happens on a device error).  A pass holds one of
// these while it works; leaving it any other way than through ok() marks the batch, whose later calls are refused
// (check_poisoned); hx_batch_destroy just synchronises.
struct Poison {
    hx_batch *b;
    bool armed = true;
    ~Poison() { if (armed) b->poisoned = true; }
    int ok() { armed = false; return 0; }
};
HX_LOCAL int check_poisoned(const hx_batch *b);

// the PCM of a pass: int16, or fp32 at int16 scale; bytes: of nframes frames of S streams
// Under PCM segments (pcm_in): p is not rows but an image, seg [S] the host's byte offsets of the streams' segments in the
// caller's image as of the call, and p stands for byte `shift` of that image - a device call's p is the image's base, a host
// call copies up only the span its segments cover (seg_span) and shifts by the span's start.
// Under PCM planes: the same with pl [S] the offsets of the streams' plane 0, pl_stride [S] (null: tight) the distance to
// plane 1, unit: an fp32 call's samples are at unit scale; the span is plane_span's.  At most one of seg and pl is set.
struct PcmIn {
    const void *p; bool f32;
    const long long *seg = nullptr; long long shift = 0;
    const long long *pl = nullptr, *pl_stride = nullptr; bool unit = false;
    bool image() const { return seg || pl; }
    int sample_bytes() const { return f32 ? (int) sizeof(float) : (int) sizeof(int16_t); }
    long long bytes(long long S, int nframes, int nchan) const { return S * nframes * 1152 * nchan * (long long) sample_bytes(); }
};
// a call's PCM argument as the batch takes it now: rows, or the segments or planes in force
static inline PcmIn pcm_in(const hx_batch *b, const void *p, bool f32)
{
    PcmIn in = {p, f32};
    if (b && !b->seg_off.empty()) in.seg = b->seg_off.data();
    else if (b && !b->pl_off.empty()) {
        in.pl = b->pl_off.data();
        in.pl_stride = b->pl_stride.empty() ? nullptr : b->pl_stride.data();
        in.unit = f32 && b->pl_unit;
    }
    return in;
}
// bytes of stream i's segment in a call of nframes: its count in force (or nframes) x 1152 x its channels as of now x sample_bytes
static inline long long seg_len(const hx_batch *b, int i, int nframes, int sample_bytes)
{
    return (long long) (b->nfr.empty() ? nframes : b->nfr[i]) * 1152 * b->params[b->cls_of[i]].nchan * sample_bytes;
}
// [lo, hi): from the lowest segment start to the highest segment end among the streams that take frames (none: lo = hi = 0)
static inline void seg_span(const hx_batch *b, int nframes, int sample_bytes, long long &lo, long long &hi)
{
    lo = LLONG_MAX; hi = 0;
    for (int i = 0; i < b->S; i++) {
        const long long n = seg_len(b, i, nframes, sample_bytes);
        if (n <= 0) continue;
        lo = std::min(lo, b->seg_off[i]);
        hi = std::max(hi, b->seg_off[i] + n);
    }
    if (lo > hi) lo = hi = 0;
}
// what a call sends up of its image's layout through img_stage: under segments [S] i64 offsets, under planes [2][S] i64,
// offsets and then strides
static inline size_t segs_stage_bytes(const hx_batch *b) { return sizeof(long long) * (size_t) b->S; }
static inline size_t planes_stage_bytes(const hx_batch *b) { return 2 * sizeof(long long) * (size_t) b->S; }
// PCM planes in force: the bytes of one plane of stream i in a call of nframes, and the distance from its plane 0 to its
// plane 1 (0 for a mono stream and for one that takes no frame: theirs is not looked at)
static inline long long plane_len(const hx_batch *b, int i, int nframes, int sample_bytes)
{
    return (long long) (b->nfr.empty() ? nframes : b->nfr[i]) * 1152 * sample_bytes;
}
static inline long long plane_stride(const hx_batch *b, int i, int nframes, int sample_bytes)
{
    const long long n = plane_len(b, i, nframes, sample_bytes);
    if (n <= 0 || b->params[b->cls_of[i]].nchan < 2) return 0;
    return b->pl_stride.empty() ? n : b->pl_stride[i];
}
// [lo, hi): from the lowest plane start to the highest plane end among the streams that take frames (none: lo = hi = 0);
// the planes in force must have passed check_planes
static inline void plane_span(const hx_batch *b, int nframes, int sample_bytes, long long &lo, long long &hi)
{
    lo = LLONG_MAX; hi = 0;
    for (int i = 0; i < b->S; i++) {
        const long long n = plane_len(b, i, nframes, sample_bytes), d = plane_stride(b, i, nframes, sample_bytes);
        if (n <= 0) continue;
        lo = std::min(lo, b->pl_off[i] + std::min(0LL, d));
        hi = std::max(hi, b->pl_off[i] + std::max(0LL, d) + n);
    }
    if (lo > hi) lo = hi = 0;
}
// the span of the image a host call copies up under segments or planes (in.image())
static inline void image_span(const hx_batch *b, const PcmIn &in, int nframes, long long &lo, long long &hi)
{
    if (in.seg) seg_span(b, nframes, in.sample_bytes(), lo, hi);
    else plane_span(b, nframes, in.sample_bytes(), lo, hi);
}
// a call that writes the caller's rows and the optional outputs set on the batch (a null batch: the argument checks refuse it)
static inline Call call_on(const hx_batch *b, unsigned char *out, long long out_stride, int *out_bytes)
{
    Call c = {out, out_stride, out_bytes, b ? b->opt : OptOut()};
    c.ledger = b ? b->d_ledger : nullptr;
    if (b) c.files = b->files;
    return c;
}
// where a pass runs: every kernel on the caller's stream, or (hx_batch_submit_*) front end and stream walk on the batch's
// own two streams, ordered by events (see hx_batch); a device-buffer submit also defers its packing
enum PassKind { PASS_PLAIN, PASS_SUBMIT_DEVICE, PASS_SUBMIT_HOST };

// Argument checks of every encode entry point, made before anything is allocated, copied or launched; check_call: ... of
// the PCM entry points, which a converting batch refuses
HX_LOCAL int check_args(const hx_batch *b, const void *in, int nframes, const void *out, long long out_stride, const void *out_bytes, bool outputs = true);
HX_LOCAL int check_call(const hx_batch *b, const void *pcm, int nframes, const void *out, long long out_stride, const void *out_bytes, bool outputs = true);
// ... of the per-stream frame counts in force against the call's nframes (check_args makes it; hx_multi for all its blocks
// before any of them starts, with `first` = the block's first stream, so the message names the caller's stream number)
HX_LOCAL int check_counts(const hx_batch *b, int nframes, int first);
// what hx_batch_frame_counts needs before it can set counts, and nothing else of it (hx_multi: all blocks, then set all)
HX_LOCAL int counts_reserve(hx_batch *b, bool buffers);
// ... the staging, events and device copies alone, and one upload of b->nfr in the plain calls' rotation on stream q (d_nfr: the
// device copy it went to) - the converting calls under counts (hx_batch_src.hip), whose k_src reads the counts before the pass
HX_LOCAL int counts_buffers(hx_batch *b);
HX_LOCAL int counts_upload_plain(hx_batch *b, hipStream_t q, const int *&d_nfr);
// PCM segments.  segs_reserve: what hx_batch_pcm_segments needs before it can set segments, and nothing else of it (hx_multi:
// all blocks, then set all) - whether the batch takes them at all and (buffers) at the first use their staging.
// check_segments: the segments in force against a call of nframes and this sample size, per stream that takes frames, before
// anything is allocated, copied or launched (none in force: 0); first: as for check_counts.  The counts in force must have
// passed check_counts.
HX_LOCAL int segs_reserve(hx_batch *b, bool buffers);
HX_LOCAL int check_segments(const hx_batch *b, int nframes, int sample_bytes, int first);
// PCM planes, the same way (none in force: 0): every plane of every stream that takes frames starts at or above 0, on a
// multiple of the sample size, and ends within in_bytes; an s16 call under unit_scale is refused.  The message names stream
// and channel.  planes_args: the setters' own argument checks (hx_multi: before one block is set).
HX_LOCAL int check_planes(const hx_batch *b, int nframes, int sample_bytes, int first);
HX_LOCAL int planes_args(const long long *off, long long in_bytes, int unit_scale);
// both, as every PCM entry point makes them
static inline int check_image(const hx_batch *b, int nframes, int sample_bytes, int first)
{
    return check_segments(b, nframes, sample_bytes, first) != 0 || check_planes(b, nframes, sample_bytes, first) != 0 ? -1 : 0;
}
// ... and the range check of counts that come as a call's argument (first: as for check_counts)
HX_LOCAL int check_counts_arg(const int *nfr, int S, int nframes, int first);
// A converting call's input extents against its rows, per stream under its count (nfr null: nframes), before anything runs;
// used_end [S] or null: where each stream's following call would start.  first: as for check_counts.
HX_LOCAL int src_extents(const hx_batch *b, long long in_stride, const long long *frame_off, int nframes, const int *nfr, int first, long long *used_end);
// ... and of the optional outputs a call would take: a CRC buffer without frame counters is refused, and so is a call
// without both that feeds a live ledger record (nfr: the call's per-stream counts or null; first: as for check_counts)
HX_LOCAL int check_opt(const hx_batch *b, const OptOut &o, const int *nfr, int first = 0);
// the counts a call made now on a plain batch would take (null: uniform)
static inline const int *counts_in_force(const hx_batch *b) { return b->nfr.empty() ? nullptr : b->nfr.data(); }
// one pass of the pipeline over the batch (arguments checked by the caller); encode_checked: check_call, then the pass
HX_LOCAL int encode_pass(hx_batch *b, PcmIn in, int nframes, const Call &c, void *stream, PassKind kind);
HX_LOCAL int encode_checked(hx_batch *b, PcmIn in, int nframes, const Call &c, void *stream, PassKind kind);
// the host-buffer PCM calls; hd: the *_host_dense calls' image, its capacity and offsets in host memory (see host_call)
struct HostDense { unsigned char *dense; long long cap; long long *off; long long bound; };
HX_LOCAL int encode_host(hx_batch *b, PcmIn in, int nframes, unsigned char *out, long long out_stride, int *out_bytes, int *stats, const HostDense *hd = nullptr,
                         unsigned short *crc = nullptr, bool files = false, float *recon = nullptr);
// decoded PCM: what hx_batch_recon_buffer refuses about the batch, and everything it allocates at the first switch-on
HX_LOCAL int recon_refused(const hx_batch *b);
HX_LOCAL int recon_reserve(hx_batch *b);
// the *_host_files calls (file images): what they need of the batch, and the PCM form
HX_LOCAL int check_files(const hx_batch *b);
HX_LOCAL int encode_host_files(hx_batch *b, PcmIn in, int nframes);
// hx_batch_file_images in two steps (hx_multi: reserve for all blocks, then commit all): images_reserve makes the refusals and
// allocates what `cap` needs into `next`, changing nothing of the batch's view; images_commit releases the old images and takes `next`
HX_LOCAL int images_reserve(hx_batch *b, long long cap, FileImages &next);
HX_LOCAL int images_commit(hx_batch *b, const FileImages &next);
HX_LOCAL void images_drop(hx_batch *b, FileImages &next);
HX_LOCAL int ledger_poll(hx_batch *b, HX_LEDGER_BRIEF *out);
// Finished files (hx_batch_slots.hip).  files_refused: what hx_batch_file_tags refuses about the files themselves (tags null:
// what the fetch of many does) - images off, a record begun without an image, a tag of another size than the slot's head room -
// for a list that has passed the slot operations' checks; entry: null, or the caller's number of entry e, and first: the block's
// first stream (hx_multi, whose blocks take parts of the caller's list: the message names the caller's entry and stream).  file_tags: hx_batch_file_tags on stream q; wait: as for assign_slots.
// The host fetch in its two halves (hx_multi: scan all blocks, decide, then bring all): files_many_scan drains, runs k_file_off
// over the list and copies the offsets to off [n + 1]; files_many_bring gathers that list into the batch's staging and copies
// the image's off[n] = total bytes to dst.
HX_LOCAL int files_refused(const hx_batch *b, const int *idx, const HX_FILE_TAG *tags, int n, const int *entry, int first);
HX_LOCAL int file_tags(hx_batch *b, const int *idx, const HX_FILE_TAG *tags, int n, void *stream, bool wait);
HX_LOCAL int files_many_scan(hx_batch *b, const int *idx, int n, long long *off);
HX_LOCAL int files_many_bring(hx_batch *b, int n, long long total, unsigned char *dst);
// The one create path (hx_batch.hip).  ec[nmenu] (and src[nmenu]: a converting batch) is the menu, cfg[nstreams] or null
// (= entry 0) the entry each slot starts with.  A refusal names the entry as "<label> <origin[j]>: " - src_label for what
// the converter rejects, cls_label for what the encoder's init or the batch's kind rejects; a null label: no prefix; a null
// origin: the entry's own number.  mixed: entries may differ in channel count (hx_batch_create_mixed); any: also in MPEG
// version and allocator generation (hx_batch_create_any).
struct MenuNames { const char *src_label, *cls_label; const int *origin; bool mixed = false, any = false; };
HX_LOCAL hx_batch *batch_create(int device, int nstreams, const HX_E_CONTROL *ec, int nmenu, const HX_SOURCE *src, const int *cfg,
                                int max_frames, const MenuNames &names);
// ... its converter parts (hx_batch_src.hip): every entry's encode control and plan (plans deduplicated), before anything
// touches the device; and the converter's buffers, sized over all plans
HX_LOCAL int src_menu(const HX_E_CONTROL *ec, const HX_SOURCE *src, int nmenu, const MenuNames &names, std::vector<HX_E_CONTROL> &ecs,
                      std::vector<HxSrcPlan> &plans, std::vector<int> &menu_plan);
HX_LOCAL int src_setup(hx_batch *b, const std::vector<HxSrcPlan> &plans);
// hx_batch_assign_streams (cfg null: hx_batch_reset_streams) on stream q; wait: behind everything in flight, and done when
// it returns
HX_LOCAL int assign_slots(hx_batch *b, const int *idx, const int *cfg, int n, void *stream, bool wait);
// hx_batch_ledger_begin on stream q (wait: as for assign_slots) and hx_batch_ledger_read (hx_multi calls them per block,
// after it has made their refusals for all blocks)
HX_LOCAL int ledger_begin(hx_batch *b, const int *idx, const HX_LEDGER_OPEN *open, int n, void *stream, bool wait);
HX_LOCAL int ledger_read(hx_batch *b, const int *idx, int n, HX_LEDGER *out);
// Slot state (hx_batch_slots.hip), set up at create: what a new stream of each class starts with, each class's blob
// fingerprint and the duplicate marks (hx_batch_create); a converting batch's per-stream plan fingerprints on the device,
// which the slot kernels check and write (hx_batch_create_src)
HX_LOCAL int slots_init(hx_batch *b);
HX_LOCAL int slots_src_init(hx_batch *b);
// make stream q wait for everything submitted so far, the deferred packing included
HX_LOCAL int order_behind_submits(hx_batch *b, hipStream_t q);
// Wait until everything enqueued on the batch is done, the deferred packing of the last device-buffer submit included.
HX_LOCAL int drain(hx_batch *b);
// the encode control of a converted source and its converter (hx_enc.cpp)
HX_LOCAL int src_encode_control(const HX_E_CONTROL *ec, int source_bits, int source_is_float, int mpeg_select, int mono_convert,
                                hx_src *conv, HX_E_CONTROL *ec_out);

// The rows of a host-buffer call from the staging d_out to the caller's `out`: in one copy, or under per-stream frame counts
// one copy per run of streams that took frames - the host row of a stream that sat the call out is not written either
// (its staging row holds an earlier call's bytes).  q: null = synchronous copies, else asynchronous on q.
// The guarantee costs copies: counts that alternate between 0 and more make S / 2 of them, one row each (4096 streams, every
// second one idle: 2048), and no gap is bridged, since that would write the idle rows in between.  The step times of uneven
// calls in DESIGN.md section 5 are of device-buffer calls and do not contain this.
static inline int rows_to_host(const hx_batch *b, unsigned char *out, const unsigned char *d_out, long long out_stride, hipStream_t q)
{
    const int S = b->S;
    for (int s = 0, e; s < S; s = e) {
        e = S;
        if (!b->nfr.empty()) {
            while (s < S && b->nfr[s] == 0) s++;
            for (e = s; e < S && b->nfr[e] > 0; e++) {}
            if (s == S) break;
        }
        const size_t at = (size_t) s * out_stride, nb = (size_t) (e - s) * out_stride;
        HIPCHK(q ? hipMemcpyAsync(out + at, d_out + at, nb, hipMemcpyDeviceToHost, q) : hipMemcpy(out + at, d_out + at, nb, hipMemcpyDeviceToHost));
    }
    return 0;
}

// One host-buffer call: grow the staging, copy the input up, make the device call `encode(c)`, wait for it and copy the
// results back.  c is the call's record: the rows are b->d_out / d_outbytes; with `stats` the call's per-frame counters
// (see hx_batch_frame_stats_buffer) go to b->d_stats and come back to the host, and the caller's device counter buffer is
// not written; with `crc` (the *_host_crc calls, which pass `stats` too) the same for the per-frame CRCs, through b->d_crc;
// every other optional output is the one set on the batch.
// drain_first: the staging may still be read by an earlier call that did not wait for its end.
// hd (the *_host_dense calls): the dense image and its offsets go to staging too, not to the caller's device image, and
// come back instead of the rows (`out` is not used): the offsets, and the image up to the last segment that fits hd->cap
// in whole - the segments that fit are a prefix of the streams, and none of them ends beyond hd->bound.
// files (the *_host_files calls; out, out_bytes, stats and crc null): rows, byte counts, counters and CRCs all go to the
// staging and stay there - the call's ledger update and file images take them from it - and what comes back is the batch's
// status word, which is the call's return value.
template <class Encode>
static int host_call(hx_batch *b, const void *in, long long in_bytes, bool drain_first, int nframes, unsigned char *out,
                     long long out_stride, int *out_bytes, int *stats, Encode encode, const HostDense *hd = nullptr, unsigned short *crc = nullptr,
                     bool files = false, float *recon = nullptr)
{
    if (!files) {   // (the optional outputs the call will take, checked before anything is allocated or copied; files: it takes both)
        OptOut o = b->opt;
        if (stats) o.frame_stats = stats;
        if (crc) o.crc = crc;
        if (check_opt(b, o, counts_in_force(b)) != 0) return -1;
    }
    HIPCHK(hipSetDevice(b->device));
    const long long obytes = (long long) b->S * out_stride, sbytes = (stats || files) ? (long long) sizeof(int) * b->S * nframes * 2 : 0;
    const long long cbytes = (crc || files) ? (long long) sizeof(unsigned short) * b->S * nframes : 0;
    if (dev_grow(b, b->d_in, b->in_cap, in_bytes) || dev_grow(b, b->d_out, b->out_cap, obytes) || dev_grow(b, b->d_stats, b->stats_cap, sbytes) ||
        dev_grow(b, b->d_crc, b->crc_cap, cbytes)) return -1;
    // (the *_host_recon calls: the decoded PCM goes to staging laid out like the input rows, and comes back below)
    const long long rrow = (long long) nframes * 1152 * b->nchan;
    if (recon && (recon_reserve(b) != 0 || dev_grow(b, b->d_reconh, b->reconh_cap, (long long) sizeof(float) * b->S * rrow))) return -1;
    if (hd && (dev_grow(b, b->d_dense, b->dense_cap, std::max(16LL, std::min(hd->cap, hd->bound))) ||
               (!b->d_dense_off && dev_alloc(b, b->d_dense_off, (long long) sizeof(long long) * (b->S + 1))))) return -1;
    if (drain_first && drain(b) != 0) return -1;
    if (in_bytes > 0) HIPCHK(hipMemcpy(b->d_in, in, (size_t) in_bytes, hipMemcpyHostToDevice));    // (0: a call under segments of which no stream takes a frame)
    Call c = call_on(b, b->d_out, out_stride, b->d_outbytes);
    if (stats || files) c.opt.frame_stats = b->d_stats;
    if (crc || files) c.opt.crc = b->d_crc;
    if (hd) c.opt.dense = DenseOut{b->d_dense, hd->cap, b->d_dense_off, nullptr};
    if (recon) c.opt.recon = b->d_reconh;
    if (encode(c) != 0 || drain(b) != 0) return -1;
    if (files) {
        int v = -1;
        HIPCHK(hipMemcpy(&v, b->d_status, sizeof(int), hipMemcpyDeviceToHost));
        return v;
    }
    HIPCHK(hipMemcpy(out_bytes, b->d_outbytes, sizeof(int) * b->S, hipMemcpyDeviceToHost));
    if (hd) {
        HIPCHK(hipMemcpy(hd->off, b->d_dense_off, sizeof(long long) * (b->S + 1), hipMemcpyDeviceToHost));
        long long k = b->S;
        while (k > 0 && hd->off[k] > hd->cap) k--;
        if (hd->off[k] > 0) HIPCHK(hipMemcpy(hd->dense, b->d_dense, (size_t) hd->off[k], hipMemcpyDeviceToHost));
    } else if (rows_to_host(b, out, b->d_out, out_stride, nullptr) != 0) return -1;
    if (stats) HIPCHK(hipMemcpy(stats, b->d_stats, (size_t) sbytes, hipMemcpyDeviceToHost));
    if (crc) HIPCHK(hipMemcpy(crc, b->d_crc, (size_t) cbytes, hipMemcpyDeviceToHost));
    // each stream's blocks of the call and no more: what lies behind them in the caller's row is not written.  One copy
    // when every stream fills its row (no counts, every stream of P channels), else one copy to the host and a trim there
    if (recon) {
        bool full = b->nfr.empty();
        for (int s = 0; full && s < b->S; s++) full = b->params[b->cls_of[s]].nchan == b->nchan;
        std::vector<float> tmp(full ? 0 : (size_t) b->S * rrow);
        HIPCHK(hipMemcpy(full ? recon : tmp.data(), b->d_reconh, sizeof(float) * (size_t) b->S * rrow, hipMemcpyDeviceToHost));
        for (int s = 0; !full && s < b->S; s++) {
            const size_t n = (size_t) (b->nfr.empty() ? nframes : b->nfr[s]) * 1152 * b->params[b->cls_of[s]].nchan;
            memcpy(recon + (size_t) s * rrow, tmp.data() + (size_t) s * rrow, sizeof(float) * n);
        }
    }
    return 0;
}
