/*
 * hmp3_amd.h - C ABI of the MI355X-native batched MP3 (MPEG-1 Layer III) encoder.
 *
 * Drop-in boundary for the Helix encoder's frame-encode path: every hx_enc_* entry point
 * replaces one public method of the reference's `class CMp3Enc`
 * (/root/reference/hmp3/src/pub/mp3enc.h:74-139), with the same argument meaning, the same
 * return values and the same error behaviour (init returns 0 on failure; encode cannot fail).
 * E_CONTROL / MPEG_HEAD / IN_OUT / INT_PAIR are the reference's plain structs
 * (pub/encapp.h:42-72,141-165; pub/mp3enc.h:66-71) and cross this ABI unchanged.
 *
 * The hx_batch_* entry points have no reference equivalent: they encode N independent streams
 * x F frames per call on one GPU, which is where the throughput comes from.  All buffers are
 * plain pointers; "device" variants take HIP device pointers and a hipStream_t (as void*).
 *
 * Everything runs on the GPU: there is no CPU fallback.  hx_batch_create / the hx_enc init calls
 * check that the device is a gfx950 (MI355X); if none is usable they return NULL / 0 and
 * hx_last_error() says why.  Every kernel launch is checked where it is made.
 */
#ifndef HMP3_AMD_H
#define HMP3_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* pub/encapp.h:42-72 */
typedef struct {
    int mode, bitrate, samprate, nsbstereo, filter_select, freq_limit, nsb_limit;
    int layer, cr_bit, original, hf_flag, vbr_flag, vbr_mnr, vbr_br_limit, vbr_delta_mnr;
    int chan_add_f0, chan_add_f1, sparse_scale;
    int mnr_adjust[21];
    int cpu_select, quick, test1, test2, test3, short_block_threshold;
} HX_E_CONTROL;

/* pub/encapp.h:141-157 */
typedef struct {
    int sync, id, option, prot, br_index, sr_index, pad, private_bit, mode, mode_ext, cr, original, emphasis;
} HX_MPEG_HEAD;

typedef struct { int in_bytes, out_bytes; } HX_IN_OUT;      /* pub/encapp.h:160-165 */
typedef struct { int a, b; } HX_INT_PAIR;                   /* pub/mp3enc.h:66-71 */

typedef struct hx_enc hx_enc;       /* one stream, CMp3Enc-compatible */
typedef struct hx_batch hx_batch;   /* N streams on one GPU */

const char *hx_last_error(void);
int hx_device_count(void);
void hx_default_control(HX_E_CONTROL *ec);                  /* CLI defaults, test/tomp3.cpp:357-384 */

/* ---- CMp3Enc replacement (one stream, host buffers) ---- */
hx_enc *hx_enc_create(int device);                          /* CMp3Enc::CMp3Enc,  mp3enc.cpp:115 */
void hx_enc_destroy(hx_enc *e);                             /* CMp3Enc::~CMp3Enc, mp3enc.cpp:201 */
/* CMp3Enc::L3_audio_encode_init (mp3enc.cpp:220): returns bytes of float PCM per call (9216) or 0 */
int hx_enc_L3_audio_encode_init(hx_enc *e, const HX_E_CONTROL *ec);
/* CMp3Enc::L3_audio_encode (mp3enc.cpp:2031): 1152 x 2 floats at int16 scale, oldest first.
   From the third call on a call is one HIP-graph launch: the encoder's single-stream chain (PCM up from page-locked staging,
   the pipeline's kernels, whose last workgroup writes byte count / frame counter / bitstream to page-locked host memory and
   publishes a sequence word behind them) is recorded once and replayed; the bytes per call are those of the plain calls.
   The *_Packet calls take the plain path; the environment variable HMP3AMD_ENC_GRAPH=0 restores it for every call. */
HX_IN_OUT hx_enc_L3_audio_encode(hx_enc *e, const float *pcm, unsigned char *bs_out);
/* CMp3Enc::MP3_audio_encode_init (mp3enc.cpp:2655): 8/16/24/32-bit PCM or 32-bit float source at
   8 - 48 kHz, converted to the encode rate by the built-in converter; returns min input bytes per call or 0 */
int hx_enc_MP3_audio_encode_init(hx_enc *e, const HX_E_CONTROL *ec, int source_bits, int source_is_float,
                                 int mpeg_select, int mono_convert);
/* CMp3Enc::MP3_audio_encode (mp3enc.cpp:2812) */
HX_IN_OUT hx_enc_MP3_audio_encode(hx_enc *e, const unsigned char *pcm, unsigned char *bs_out);
/* (init returns the bytes a call needs buffered - 1153 sample frames when no rate conversion is involved -
   and in_bytes of a call is what the converter consumed; mpeg_select: 0 track the input rate, 1 an MPEG-1
   rate, 2 an MPEG-2 rate, else the encode rate in Hz) */
int hx_enc_get_bitrate(hx_enc *e);                          /* mp3enc.cpp:3444 */
float hx_enc_get_bitrate_float(hx_enc *e);                  /* mp3enc.cpp:3451 */
float hx_enc_get_bitrate2_float(hx_enc *e);                 /* mp3enc.cpp:3468 */
unsigned hx_enc_get_frames(hx_enc *e);                      /* mp3enc.cpp:3484 */
HX_INT_PAIR hx_enc_get_frames_bytes(hx_enc *e);             /* mp3enc.cpp:3512 */
void hx_enc_info_ec(hx_enc *e, HX_E_CONTROL *ec);           /* mp3enc.cpp:3491 */
void hx_enc_info_head(hx_enc *e, HX_MPEG_HEAD *head);       /* mp3enc.cpp:3498 */
/* pub/mp3enc.h:110-131 *_Packet: also return this call's frame as a self-contained ("reformatted")
   packet: header, side info with main_data_begin 0, unpadded main data; nbytes_out[0] = its size,
   nbytes_out[1] = 0.  At the MPEG-2 rates (16 / 22.05 / 24 kHz) a call yields two single-granule
   frames (mp3enc.cpp:3301-3440): two packets back to back, nbytes_out[0] then nbytes_out[1] bytes.
   bs_out or packet may be NULL.  As in the reference, a call with bs_out NULL returns out_bytes 0 and its frames are
   counted as sent while their bytes are not (mp3enc.cpp:2964-2994); a call with packet NULL leaves nbytes_out alone. */
HX_IN_OUT hx_enc_L3_audio_encode_Packet(hx_enc *e, const float *pcm, unsigned char *bs_out, unsigned char *packet, int nbytes_out[2]);
HX_IN_OUT hx_enc_MP3_audio_encode_Packet(hx_enc *e, const unsigned char *pcm, unsigned char *bs_out, unsigned char *packet, int nbytes_out[2]);
void hx_enc_info_string(hx_enc *e, char *s);                /* mp3enc.cpp:3505, <= 80 chars */
/* CMp3Enc::out_stats (mp3enc.cpp:3522, "test routine"): the allocator's counters to stderr - the long-block
   allocator's call count; the reference's remaining columns are uninitialised diagnostics and print as 0 */
void hx_enc_out_stats(hx_enc *e);

/* ---- sample-format / sample-rate converter (host side) ----
   What CMp3Enc::MP3_audio_encode runs in front of every frame: Csrc (pub/srcc.h:87-97).  hx_enc_MP3_audio_encode
   uses it internally.  Batched callers (hx_batch_* and hx_multi_*) whose sources are at other rates or in other formats
   use the converting batches instead (hx_batch_create_src, hx_multi_create_src below), which run the same converter on
   the GPU. */
typedef struct hx_src hx_src;
hx_src *hx_src_create(void);
void hx_src_destroy(hx_src *s);
/* Csrc::sr_convert_init (srcc.cpp:730): bytes to hold per convert call, 0 = unsupported pair */
int hx_src_init(hx_src *s, int source, int channels, int bits, int is_float, int target, int target_channels,
                int *encode_cutoff_freq);
/* Csrc::sr_convert (srcc.cpp:795): 1152 samples per output channel, fp32 at int16 scale; returns input bytes used */
int hx_src_convert(hx_src *s, const unsigned char *xin, float *yout, int *out_bytes);
/* host only, changes nothing: the input bytes each of the next nframes calls of a converter that has made `calls` calls
   consumes (the in_bytes of those hx_src_convert calls; in_bytes may be NULL); returns the bytes those calls read,
   counted from the first unconsumed byte (-1: not initialised) */
long long hx_src_schedule(const hx_src *s, long long calls, int nframes, long long *in_bytes);
/* the other arguments of CMp3Enc::MP3_audio_encode_init (mp3enc.cpp:2655) for one source */
typedef struct { int bits, is_float, mpeg_select, mono_convert; } HX_SOURCE;
/* host only: the control the encoder runs behind the converter for a source (ec: samprate = the source's rate,
   mode 3 = a mono source) - what MP3_audio_encode_init derives; returns its bytes per call, 0 = rejected */
int hx_src_encode_control(const HX_E_CONTROL *ec, const HX_SOURCE *src, HX_E_CONTROL *ec_out);

/* ---- batched encode (N independent streams) ---- */
/* ec: nstreams controls, or one shared control when shared_control != 0.
   max_frames: largest nframes any later call will pass.  Returns NULL on failure. */
hx_batch *hx_batch_create(int device, int nstreams, const HX_E_CONTROL *ec, int shared_control, int max_frames);
void hx_batch_destroy(hx_batch *b);
int hx_batch_nstreams(const hx_batch *b);
/* start a new stream in slot i with the slot's configuration (the state CMp3Enc::L3_audio_encode_init leaves,
   mp3enc.cpp:278-287, 788-837); waits for work in flight, leaves the other streams alone.  It is the one-slot form of
   hx_batch_reset_streams below - the same launch, the same refusals - made synchronous: done when it returns.  Like the
   list call it zeroes the slot's three carried subband granules and not the rest of its subband rows, which no kernel
   reads before a later call has rewritten them: the output is a new batch's, and the one place where the slot differs
   from a new batch's is the "sb" debug tap beyond the carry. */
int hx_batch_reset_stream(hx_batch *b, int i);
/* checkpoint / resume of one stream (header + encoder state + subband carry, hx_batch_stream_state_bytes bytes):
   what is saved from slot i continues, after hx_batch_set_stream_state, in any slot of any batch created with
   the same control for that slot (any size, any max_frames) - another GPU or a later process included.  src
   must hold hx_batch_stream_state_bytes bytes; a blob of another library build or saved under another
   control is refused (-1, hx_last_error), on the host, before anything is copied or launched.
   The two calls are the one-slot form of hx_batch_get / set_stream_states below (one launch, one copy, the same
   refusals), except that dst / src hold hx_batch_stream_state_bytes bytes, not the list calls' stride: no byte beyond
   them is read or written. */
long long hx_batch_stream_state_bytes(const hx_batch *b);
int hx_batch_get_stream_state(hx_batch *b, int i, void *dst);
int hx_batch_set_stream_state(hx_batch *b, int i, const void *src);
/* ---- slot operations in stream order: reset, save, restore many streams at once (no reference equivalent) ----
   The three calls above serve one slot each and wait for everything in flight.  These take a list of slots, do their work
   in one kernel launch whatever n is, and are enqueued like a plain device call - a long-lived batch recycles slots between
   two pipelined submits without a wait.
   idx: HOST array of n distinct slots, copied by the call.  A blob array is [n][blob_stride] bytes; blob e belongs to
   idx[e], not to the slot number.  Its first hx_batch_stream_state_bytes bytes are byte for byte what
   hx_batch_get_stream_state writes for that slot, the bytes from there to blob_stride are written as zero, and nothing
   at or beyond n * blob_stride is written.  blob_stride: a multiple of 16 and at least hx_batch_stream_state_bytes;
   hx_batch_stream_states_stride is the smallest one.  A device blob array starts on a 16-byte boundary.
   hx_batch_reset_streams: every listed slot starts a new stream of its configuration, as hx_batch_reset_stream does
   (of a converting batch the converter too: its call count is 0 when the call returns, so hx_batch_src_schedule answers
   as on a new batch).  The other slots are not touched.
   Ordering: an operation is ordered like a plain device call.  It runs on `stream` behind everything the batch has in
   flight.  After pipelined submits it first enqueues the packing that the last submit left for later - ungated, exactly
   as hx_batch_wait does: that submit's output buffers must still be valid, and the batch is no longer "in flight"
   afterwards.  Calls made on the batch afterwards see its effect under the same rule as plain calls: on the same stream,
   or on streams the caller orders behind it.  Between two submits an operation costs that one step's packing overlap, and
   nothing else.
   Host waits: none but the staging's.  The list travels to the device through one of three page-locked staging copies:
   an operation waits on the host until the operation three before it is done, which can be as long as the work that one
   was ordered behind, and it cannot be made while its stream is being captured into a graph.
   Refusals (-1, before anything is allocated, uploaded or launched; hx_last_error names the entry; the batch stays usable
   and unchanged): a null batch, n < 0, a null idx with n > 0; a slot out of range or listed twice; a blob_stride below
   hx_batch_stream_state_bytes or not a multiple of 16; a null blob array with n > 0, a device blob array that is not
   16-byte aligned; a batch that became unusable.  n = 0 returns 0 and launches nothing.
   Restored blobs: hx_batch_set_stream_states checks all n headers on the host first, with hx_batch_set_stream_state's
   messages, and restores all slots or (-1) none.  hx_batch_set_stream_states_device cannot know: its kernel checks each
   blob's header {magic of the batch's kind, format version, state size, configuration fingerprint of the slot}; a blob
   that fails leaves its slot untouched and sets status bit 32 (hx_batch_status), the other listed slots are restored.
   A restored stream's class index is the receiving batch's, as with hx_batch_set_stream_state.
   The host-blob calls are synchronous (they wait for the work in flight), and make one gather / scatter launch and one
   copy whatever n is; the single-slot calls are their n = 1 case.  On converting batches they carry the converter part.
   Not covered: device blobs of converting batches - the two *_states_device calls return -1 there, because the host's
   converter call counts are authoritative for hx_batch_src_schedule and the extent checks and a device blob cannot
   update them without a wait; hx_multi_* (use hx_multi_batch), the hx_enc_* encoder and the command-line tool. */
/* blob_stride of the calls below: hx_batch_stream_state_bytes rounded up to 16 */
long long hx_batch_stream_states_stride(const hx_batch *b);
/* idx: HOST array of n distinct slots, copied by the call.  Asynchronous on `stream`. */
int hx_batch_reset_streams(hx_batch *b, const int *idx, int n, void *stream);
int hx_batch_get_stream_states_device(hx_batch *b, const int *idx, int n, void *d_blobs, long long blob_stride, void *stream);
int hx_batch_set_stream_states_device(hx_batch *b, const int *idx, int n, const void *d_blobs, long long blob_stride, void *stream);
/* host blobs, synchronous: one gather / scatter launch and one copy, whatever n is */
int hx_batch_get_stream_states(hx_batch *b, const int *idx, int n, void *blobs, long long blob_stride);
int hx_batch_set_stream_states(hx_batch *b, const int *idx, int n, const void *blobs, long long blob_stride);
/* ---- slot configurations: a freed slot takes a stream of any control of the batch's menu (no reference equivalent) ----
   A batch created with hx_batch_create / hx_batch_create_src ties every slot to the control it was created with: a slot whose
   44.1 kHz CBR file has ended takes another 44.1 kHz CBR file and nothing else.  A menu lifts that: the batch is created with
   the nmenu configurations it will ever run, every slot starts on one of them, and hx_batch_assign_streams hands listed slots
   other entries in stream order.
   The menu: ec[nmenu]; src NULL = a plain batch, else src[nmenu] = a converting batch whose entry j is the pair (ec[j], src[j])
   as hx_batch_create_src takes them.  cfg: [nstreams] the entry each slot starts with, NULL = entry 0 for all.
   Everything create sizes or decides from the batch's configurations is taken over the whole menu, whichever entries the slots
   start with: the DC-blocker's PCM staging, the choice of the stream-walk build, hx_batch_out_stride, the parameter and
   initial-state tables and the blob fingerprints; of a converting batch the plan table, the plans' fingerprints, the
   converter's LDS layout and hx_batch_src_in_stride.
   A batch is still of one kind: entries that differ in channel count, in MPEG-1 / MPEG-2 rates or in allocator generation are
   refused at create with hx_batch_create's messages, and so is an entry the reference's init or the converter rejects;
   hx_last_error names it ("menu entry 2: ...").  Identical entries are allowed, and hx_batch_stream_config returns the
   caller's index whatever they share internally.  hx_batch_create and hx_batch_create_src are the case whose menu is their
   distinct controls (control / source pairs) in order of first appearance; hx_batch_nconfigs counts those.
   The menu is fixed for the batch's life: entries cannot be added after create.
   hx_batch_assign_streams: slot idx[e] starts a new stream of menu entry cfg[e].  Its contract is hx_batch_reset_streams' word
   for word - one launch whatever n is, ordered like a plain device call behind everything the batch has in flight (the
   deferred packing of the last submit goes out first, ungated), the list through the slot operations' staging rotation, no
   host wait but that rotation's, not under stream capture, the other slots untouched, n = 0 returns 0 and launches nothing,
   and the same refusals before anything is allocated, uploaded or launched, plus a null cfg with n > 0 and
   "entry e: configuration c out of range".  With cfg[e] equal to the slot's present entry it is hx_batch_reset_streams for
   that slot: the two are one implementation.
   After the call slot idx[e] produces, from its next frame on, exactly the bytes of slot 0 of a new batch created with
   ec[cfg[e]] (and src[cfg[e]]): rows, out_bytes, packets, frame counters, MusicCRC, dense image and checkpoint blob.
   The host's view of the slot moves when the call is made, as the converter's call count does at a reset: from the call's
   return on hx_batch_stream_config, hx_batch_src_schedule, the extent checks of later converting calls, the host-blob
   restores' header checks and the entries of later slot operations are the new entry's.  The device follows in stream order.
   Converter: the carried case-4 samples of the slot's previous occupant stay where they are; a stream's call 0 reads none
   under any plan.
   Restoring a blob into a slot that runs another entry stays refused (on the host by hx_batch_set_stream_states, with status
   bit 32 by the device form).  The way to do it is to assign, then restore: two calls, two launches.  There is no call that
   adopts whatever configuration a blob carries.
   hx_multi_assign_streams: the same over all blocks; idx counts streams over all blocks.  Synchronous like the other
   hx_multi calls; every refusal is made for all blocks before one of them starts: all blocks or (-1) none.
   The checkpoint blob of an assigned slot is a new batch's but for one word: the class index at the start of the stream
   record is the batch's own numbering of its menu's configurations, which a restore replaces with the receiving batch's.
   The command-line tool's -batch -slots<n> runs any number of files through n slots this way.
   Not covered: entries added after create; device blobs and pipelined submits of converting batches, as before.  (Entries
   of different channel counts: hx_batch_create_mixed below; of different MPEG versions or allocator generations:
   hx_batch_create_any below.) */
hx_batch *hx_batch_create_menu(int device, int nstreams, const HX_E_CONTROL *ec, int nmenu, const HX_SOURCE *src,
                               const int *cfg, int max_frames);
int hx_batch_nconfigs(const hx_batch *b);
int hx_batch_stream_config(const hx_batch *b, int i);      /* the entry slot i runs as of the calls made so far; -1 bad arguments */
/* slot idx[e] starts a new stream of menu entry cfg[e]; idx, cfg: HOST arrays of n, copied by the call; asynchronous on `stream` */
int hx_batch_assign_streams(hx_batch *b, const int *idx, const int *cfg, int n, void *stream);
/* ---- mixed batches: mono and stereo streams share one batch and one menu (no reference equivalent) ----
   hx_batch_create_mixed is hx_batch_create_menu word for word, except that its entries may differ in channel count: mode 3
   (mono) beside the stereo modes; of a converting batch the converter's output channels, so a mono source, a stereo source and
   a stereo source with mono_convert share a batch.  The three other create calls keep refusing that, with their messages.
   Row pitch: P = hx_batch_pcm_channels = the largest channel count over the menu.  The PCM of every plain encode / submit call
   (device and host buffers, s16 and f32, *_stats, *_crc, *_host_dense) is [nstreams][nframes * 1152 * P] samples.  A stream of
   P channels fills its row interleaved, as in any batch.
   A mono stream of a P = 2 batch: its nframes * 1152 samples sit contiguous at the start of its row (under per-stream frame
   counts: the first n * 1152).  The rest of the row has no influence on any output or state and may be uninitialised.
   A uniform menu: P is that channel count, and the batch is in every respect what hx_batch_create_menu returns for the same
   arguments - same layout, same bytes, same kernel choice.
   Sizing: everything create sizes from the configurations is taken over the whole menu as for any menu (hx_batch_out_stride,
   the DC blocker's staging, hx_batch_src_in_stride, the converter's LDS layout, the choice of the stream-walk build); what is
   sized by a channel count is sized by P.  A host-fed mono stream of a P = 2 batch therefore moves the unused half of its
   row over the link with the rest (unless the call is fed an image: "PCM segments" below).
   hx_batch_assign_streams / hx_multi_assign_streams move a slot between a mono and a stereo entry under their contract above,
   unchanged: from its next frame on the slot produces exactly the bytes of slot 0 of a new batch created with that entry -
   rows, out_bytes, packets, frame counters, MusicCRC, dense image and checkpoint blob (but for the class index word).
   Converting batches: the input rows are bytes and per stream already.  The converted PCM (the "srcpcm" tap) takes the
   layout above: row pitch nframes * 1152 * P floats, a mono stream's frames contiguous at the row's start.
   Checkpoint blobs are those of any batch and interchangeable with them: a mono stream saved from a mixed batch restores
   into a uniform mono batch of the same control, and back (the fingerprint is per control and holds the channel count).
   Still refused at create, with hx_batch_create's messages ("menu entry j: ..."): MPEG-1 with MPEG-2 rates, and the two
   allocator generations - dual channel (mode 2) and intensity stereo stay apart from the others (hx_batch_create_any below
   takes them).
   hx_batch_frames_bytes, the ledger (frames_per_call is the MPEG version of the entry the slot runs), hx_batch_nconfigs and
   hx_batch_stream_config are what they are for any menu.
   hx_multi_create_mixed: the same in blocks over several devices; every block gets the whole menu and so the same P, and the
   caller's PCM is split between the blocks by P. */
hx_batch *hx_batch_create_mixed(int device, int nstreams, const HX_E_CONTROL *ec, int nmenu, const HX_SOURCE *src,
                                const int *cfg, int max_frames);
int hx_batch_pcm_channels(const hx_batch *b);              /* P: the channel count the PCM rows are pitched for = the largest over the menu */
int hx_batch_stream_channels(const hx_batch *b, int i);    /* channels of the entry slot i runs as of the calls made so far; -1 bad arguments */
/* ---- one batch for every stream kind: MPEG-1 and MPEG-2 rates, both allocator generations (no reference equivalent) ----
   hx_batch_create_any is hx_batch_create_mixed word for word, except that its entries may also differ in MPEG version (the
   MPEG-1 rates 32 / 44.1 / 48 kHz beside the MPEG-2 rates 16 / 22.05 / 24 kHz) and in allocator generation (dual channel,
   mode 2, and intensity stereo beside the others).  The four other create calls keep refusing that, with their messages.
   An entry's kind is 2 * (first-generation allocator) + (MPEG-2 rate).  A menu of one kind gives a batch that is in every
   respect what hx_batch_create_mixed returns for the same arguments: same kernel choice, same launches, same bytes.
   Input: a call's PCM is nframes blocks of 1152 samples per channel for every stream, whatever its rate; the row layout is
   hx_batch_create_mixed's.  Of a block an MPEG-1 stream makes one frame, an MPEG-2 stream two: hx_batch_stream_frames_per_block
   says which for the entry a slot runs as of the calls made so far; callers size their hx_batch_frames_bytes-style
   bookkeeping from it.  Everything that counts per call - nframes, per-stream frame counts, frame counters, packets, CRCs,
   the ledger's ncalls - counts input blocks for every stream.
   hx_batch_out_stride is the largest over the menu's classes of (frames per block * nframes + 2) * the class's largest frame
   + 4096, rounded up to 256; for a menu of one MPEG version that is what it always was.
   Per slot, every contract stands as it is: hx_batch_assign_streams / hx_multi_assign_streams between entries of any kinds
   (from its next frame on the slot produces exactly the bytes of slot 0 of a new batch created with that entry); reset,
   save and restore in their host and device forms (a blob is its control's, whatever batch saved it); per-stream frame
   counts; packets - an MPEG-2 stream's two packet sizes per block sit beside an MPEG-1 stream's {size, 0}; frame counters,
   MusicCRC and the dense image; the ledger, whose frames_per_call is that of the entry the slot runs when
   hx_batch_ledger_begin is called; converting batches - one 44.1 kHz source may feed a 22.05 kHz entry beside a 44.1 kHz
   one; pipelined submits of plain batches.
   The stream walk of a batch of several kinds is one launch per kind that has streams, one after the other: hx_batch_alloc_kernel_ms
   covers them all.  The low-footprint build (HMP3AMD_K6) is chosen for the kind-0 streams by the usual rule, which counts
   all of the batch's streams against the resident set, not the kind-0 streams alone: a large batch with few kind-0 streams
   walks those few with the low-footprint build, slower per stream, for no gain - HMP3AMD_K6=fat overrides it.
   hx_multi_create_any: the same in blocks over several devices; every block gets the whole menu, so the blocks agree in
   row pitch and out_stride whichever entries their slots start with. */
hx_batch *hx_batch_create_any(int device, int nstreams, const HX_E_CONTROL *ec, int nmenu, const HX_SOURCE *src,
                              const int *cfg, int max_frames);
int hx_batch_stream_frames_per_block(const hx_batch *b, int i);   /* 1 or 2: frames per 1152-sample block of the entry slot i runs as of the calls made so far; -1 bad arguments */
/* worst-case bytes one stream can emit in a call of nframes frames */
long long hx_batch_out_stride(const hx_batch *b, int nframes);
/* PCM: int16 interleaved L/R, [nstreams][nframes*1152][2]; out: [nstreams][out_stride] bytes;
   out_bytes: [nstreams] bytes produced (whole frames; the frames emitted are exactly those the
   reference emits over the same nframes calls).  stream: hipStream_t or NULL.
   Asynchronous on `stream`.  Returns 0, or a negative error. */
int hx_batch_encode_s16_device(hx_batch *b, const int16_t *d_pcm, int nframes, unsigned char *d_out,
                               long long out_stride, int *d_out_bytes, void *stream);
/* same with host buffers (staged through the device, synchronous) */
int hx_batch_encode_s16_host(hx_batch *b, const int16_t *pcm, int nframes, unsigned char *out,
                             long long out_stride, int *out_bytes);
/* the same for fp32 PCM at int16 scale (+-32768), the form CMp3Enc::L3_audio_encode takes
   (pub/mp3enc.h:90-98; a1 of the path: srcc.cpp:805-808 scales [-1,1) floats by 32768 first).
   Samples are not limited to that scale: the bytes are the reference's for any finite value, and the tests check it from
   float32's subnormal range (which the kernels keep: no flush to zero) up to 2^16 x full scale.  NaN and infinite samples
   are outside what the reference defines. */
int hx_batch_encode_f32_device(hx_batch *b, const float *d_pcm, int nframes, unsigned char *d_out,
                               long long out_stride, int *d_out_bytes, void *stream);
int hx_batch_encode_f32_host(hx_batch *b, const float *pcm, int nframes, unsigned char *out,
                             long long out_stride, int *out_bytes);
/* Pipelined form of the device calls (no reference equivalent: the reference encodes one frame per
   call on the CPU).  A submit is asynchronous like the plain call, but its outputs are ordered on
   `stream` only by a later hx_batch_wait (or by the next plain / host-buffer call on the batch); the
   PCM must be ready on `stream` at the submit and stay unchanged until hx_batch_wait.  Consecutive
   submits overlap: the front-end kernels of call n+1 and the bit packing of call n-1 run on the SIMDs
   that the allocator kernel of call n leaves idle while its slowest streams finish.  Hand consecutive
   submits different d_out / d_out_bytes (two sets in turn): with overlapping ones the result is the
   same, but the allocator launch waits for the previous call's packing.
   hx_batch_wait enqueues the packing that the last submit left for later: it writes that submit's d_out and, where
   packet outputs were on at the submit, that submit's packet buffer - they must still be valid then. */
int hx_batch_submit_s16_device(hx_batch *b, const int16_t *d_pcm, int nframes, unsigned char *d_out,
                               long long out_stride, int *d_out_bytes, void *stream);
int hx_batch_submit_f32_device(hx_batch *b, const float *d_pcm, int nframes, unsigned char *d_out,
                               long long out_stride, int *d_out_bytes, void *stream);
int hx_batch_wait(hx_batch *b, void *stream);
/* a submit's front end is held back until the previous call's allocator kernel occupies its share of the chip:
   until this percentage (default 90) of the workgroups the device can hold at once have started.  It then
   queues for the slots that finishing streams free and runs in that kernel's tail; 0 releases it at once. */
void hx_batch_set_gate(hx_batch *b, int percent);
/* The same pipelining for host buffers: the PCM of call n+1 crosses PCIe while call n is encoded and the
   bitstream of call n while call n+1 is.  pcm must stay unchanged, and out / out_bytes are undefined, until
   hx_batch_wait_host returns.  Use page-locked memory (hx_pinned_alloc) for copies that really overlap. */
int hx_batch_submit_s16_host(hx_batch *b, const int16_t *pcm, int nframes, unsigned char *out, long long out_stride, int *out_bytes);
int hx_batch_submit_f32_host(hx_batch *b, const float *pcm, int nframes, unsigned char *out, long long out_stride, int *out_bytes);
int hx_batch_wait_host(hx_batch *b);
void *hx_pinned_alloc(long long bytes);
void hx_pinned_free(void *p);
/* optional packet outputs of the batched calls: d_packet [nstreams][nframes][frame_stride] bytes,
   d_packet_bytes [nstreams][nframes][2] (the reference's nbytes_out[2] of every call: {size, 0},
   or the sizes of the two back-to-back packets of an MPEG-2 call); frame_stride >= the packet
   bytes of one call (4096 is always enough).  NULL switches them off.  Applies to the calls
   that follow: a call writes the buffers in force when it is made - a submit too, all of whose
   packet output (sizes, headers, side info and the main data its deferred packing adds) goes to the
   buffers set at the submit, whatever is set or switched off afterwards.  Like d_out they must stay
   valid until the hx_batch_wait behind the submit.  Consecutive submits take different packet
   buffers (two sets in turn, like d_out): a submit's stream walk writes its packets' headers while
   the previous submit's packing may still be writing main data, and nothing orders the two. */
void hx_batch_packet_buffers(hx_batch *b, unsigned char *d_packet, long long frame_stride, int *d_packet_bytes);
/* optional per-frame counters of the batched calls: d_stats [nstreams][nframes][2] = the stream's
   get_frames() / bytes emitted so far after each input frame, i.e. what a caller of the per-frame
   API (CMp3Enc::L3_audio_encode_get_frames_bytes after every call) would have seen.  NULL = off.
   Applies to the calls that follow; a call writes the buffer in force when it is made. */
void hx_batch_frame_stats_buffer(hx_batch *b, int *d_stats);
/* fp32 host call that also returns those counters to a host array stats[nstreams][nframes][2] */
int hx_batch_encode_f32_host_stats(hx_batch *b, const float *pcm, int nframes, unsigned char *out,
                                   long long out_stride, int *out_bytes, int *stats);
/* ---- MusicCRC: the CRC-16 of a call's bitstreams, per stream and input frame (no reference equivalent; the value is
   xhead.c's XingHeaderUpdateCRC) ----
   The Xing / Info / LAME tag carries a CRC over every audio byte of the file.  A call's CRC output is stateless - the CRC
   of THIS call's bytes from seed 0 - and the host joins calls with hx_xing_crc_combine: no CRC state in the stream-state
   blob (its size and format are unchanged), no ordering question between pipelined submits, no special case for
   hx_batch_reset_stream.
   d_crc [nstreams][nframes] unsigned short.  With e[f] = the bytes of row i that the stream had emitted in THIS call
   after input frame f (e[nframes-1] = out_bytes[i]; e[f] = out_bytes[i] - (stats[nframes-1][1] - stats[f][1]) in
   unsigned arithmetic), d_crc[i][f] = hx_xing_update_crc(0, row i, e[f]); e[f] = 0 gives 0.  NULL = off (nothing is
   launched for it).  d_crc must be 2-byte aligned (else -1).
   Applies to the calls that follow; a call writes the buffer in force when it is made - a submit too: the CRC kernel
   travels with its deferred packing, d_crc (and the frame counters it reads) must stay valid until the hx_batch_wait
   behind the submit, and consecutive submits take different buffers (two in turn, like d_out).
   A CRC call needs a frame-counter buffer (hx_batch_frame_stats_buffer) in force, because e[f] comes from it: a call
   with d_crc set and no frame counters is refused (-1, hx_last_error) before anything runs, and the batch stays usable.
   The rows, out_bytes, packets, counters and the dense image are written exactly as without it, by every kind of batch
   (MPEG-1 and MPEG-2, both builds of the rate-loop kernel, the first-generation allocator, converting batches through
   hx_batch_encode_src_device).
   The converting host calls return it through the crc argument of hx_batch_encode_src_counts_host and
   hx_multi_encode_src_counts_host (nfr = NULL for a uniform call); hx_batch_encode_src_host and hx_multi_encode_src_host
   themselves have no CRC argument (a CRC buffer set on a converting batch is written by them like any other optional
   output).
   Not covered: the per-frame hx_enc_* calls keep the host function hx_xing_update_crc. */
int hx_batch_crc_buffer(hx_batch *b, unsigned short *d_crc);
/* fp32 host call that returns the counters and the CRCs to host arrays stats[nstreams][nframes][2] and
   crc[nstreams][nframes]; both are required */
int hx_batch_encode_f32_host_crc(hx_batch *b, const float *pcm, int nframes, unsigned char *out, long long out_stride,
                                 int *out_bytes, int *stats, unsigned short *crc);
/* ---- decoded PCM: a call's frames reconstructed on the GPU (no reference equivalent: the reference has no decoder) ----
   For every stream and every 1152-sample input block of a call, the 1152 samples per channel that an ISO 11172-3 decoder
   outputs for the frame the encoder coded from that block: float at int16 scale, neither clipped nor rounded.  It is
   computed from what the stream walk hands to the packing (quantised lines, signs, scalefactors, side information), not
   from the bytes; the decoder's steps are requantisation, M/S, reorder of short blocks, alias reduction, IMDCT with the
   block-type windows, overlap-add, frequency inversion and polyphase synthesis.
   Layout: d_recon [nstreams][nframes * 1152 * P] float, P = hx_batch_pcm_channels(b) - exactly the layout of the f32 PCM
   rows (a stream of P channels interleaved, a mono stream of a P = 2 batch contiguous at the start of its row), so a recon
   row can be fed straight back as input.  d_recon must be 4-byte aligned (else -1).  NULL = off: nothing is launched for
   it, and before the first switch-on nothing is allocated for it.
   Meaning: call c of a stream codes frame c of its bitstream, and block f of the row is the decoder's output for that
   frame given the decoder's state after the stream's earlier frames: concatenated over calls, a stream's recon is what a
   decoder outputs for its concatenated bitstream.  It trails the input by D = hx_recon_delay() = 2209 samples: the 1680
   of the encoder that the file tag carries (1152 of look-ahead and the analysis side of the filter banks) and the
   decoder's 529.  Recon is tied to what a call codes, not to what it emits: the bit reservoir may hold a frame's bytes
   back for several calls, its recon is there at once.
   State: per stream the previous granule's IMDCT tails and the last 15 time slots of hybrid output per channel, about
   8 KB, in an array of the batch made at the first switch-on - outside the stream state: hx_batch_get / set_stream_state
   blobs, their size and HX_STATE_VERSION are unchanged.  A new batch starts from zero state; hx_batch_reset_streams,
   hx_batch_assign_streams and every hx_batch_set_stream_state* call (an accepted blob) zero it for the listed slots, in
   stream order.  The state advances only with calls that have a
   recon buffer in force.
   Determinism: a sample depends on its stream's own records only, every value is formed in one fixed operation order and
   the state is carried as the floats themselves, so recon is bit-identical however the frames are split over calls,
   whichever slot and batch size the stream runs in, on either build of the stream walk, on plain calls and submits.
   Per-stream frame counts: blocks f < n are written, blocks f >= n are not touched; n = 0 leaves the state unchanged.
   Submits: the kernels travel with the submit's deferred packing; a submit writes the buffer in force when it was made,
   the buffer is valid after the hx_batch_wait behind it, and consecutive submits take two buffers in turn.
   Honoured by every encode and submit entry point of a plain batch and by hx_batch_encode_src_device and its counts
   form.  The rows, out_bytes, packets, counters, CRCs, dense image, ledger and file images are byte for byte what they
   are without it.  While it is on, the stream walk writes a frame record per frame (one lane, cold code): DESIGN.md has
   the cost.  With the debug taps on as well (hx_batch_debug_enable), a plain call's frame records serve both; a submit's
   go to an array of its own buffer set, so the "dbg" tap is not written for a submit made with recon on.
   Refused by the setter (-1, hx_last_error): a null batch, a misaligned pointer, and a batch whose menu holds a class
   that is not MPEG-1 on the second-generation allocator (an MPEG-2 rate, intensity stereo, dual channel): the message
   names the class.  The stream walk's frame record lacks what those need (the first MPEG-2 frame's ms, intensity positions).
   Not covered: those kinds; recon state in the checkpoint blob - a restored stream continues from ZERO recon state, so
   the first two granules after hx_batch_set_stream_state carry a transient; hx_multi_*; the hx_enc_* encoder; the
   command line. */
int hx_batch_recon_buffer(hx_batch *b, float *d_recon);
/* fp32 host call that returns the call's recon to a host array recon[nstreams][nframes * 1152 * P] (each stream's blocks
   of the call and nothing behind them); a recon buffer set on the batch is not written by it */
int hx_batch_encode_f32_host_recon(hx_batch *b, const float *pcm, int nframes, unsigned char *out, long long out_stride,
                                   int *out_bytes, float *recon);
/* D: the samples recon trails the input by, a constant of this encoder / decoder pair */
int hx_recon_delay(void);
/* ---- per-stream frame counts: each stream of a call advances on its own (no reference equivalent; per stream it is the
   reference called nfr[i] times) ----
   nfr: HOST array [nstreams], copied by this function; NULL = every stream takes the call's nframes (the default).
   Returns 0 / -1.  Sticky like the other per-batch setters; a call takes the counts in force when it is made - a submit
   too: its deferred packing works with the counts of its own submit whatever is set afterwards.  Honoured by every encode
   and submit entry point of a plain batch, device and host buffers, and by hx_multi_encode_*_host*.  With n = nfr[i]:
     - a call with any n < 0 or n > nframes is refused (-1, hx_last_error names the stream) before anything is allocated,
       copied or launched; the batch stays usable;
     - the input layout is unchanged, [nstreams][nframes*1152][nch]: stream i's input is the first n*1152 samples of its
       row, and the rest of the row has no influence on any output or state (it may be uninitialised);
     - row i and out_bytes[i] hold exactly what the reference emits over those n calls; hx_batch_out_stride(b, nframes)
       remains the bound;
     - n = 0: out_bytes[i] = 0, row i is not written, and the stream's checkpoint (hx_batch_get_stream_state) is
       bit-identical before and after the call - an idle slot of a long-lived batch sits the call out (row i: of the
       device calls the device row, of the host-buffer calls the caller's host row, which is left out of the copy back);
     - optional outputs: entries f < n are as without counts; frame counters at f >= n repeat the stream's counters as
       they stand at the end of the call (n = 0: those it entered with); packet sizes at f >= n are {0, 0} and the packet
       bytes there are not written; the MusicCRC follows from the counters by its e[f] formula, so d_crc[i][f >= n] is
       the CRC of the whole of this call's row i; the dense image follows out_bytes.
   The counts travel to the device through one of three page-locked staging copies: a call under counts waits on the
   host until the upload of the third call before it is done, which can be as long as the earlier calls' kernels on that
   stream take, and it cannot be made while its stream is being captured into a graph.  Calls without counts do neither.
   The setter either sets the counts or (-1) changes nothing, and leaves the calling thread's current device alone.
   Converting batches take their counts per call, as an argument of hx_batch_encode_src_counts_* (below, with their
   contract); this setter returns -1 on a converting batch.
   Not covered: the hx_enc_* encoder, and bench.py, which measures uniform calls. */
int hx_batch_frame_counts(hx_batch *b, const int *nfr);
/* ---- PCM segments: a call's input packed back to back, spread on the GPU (no reference equivalent) ----
   The rows [nstreams][nframes * 1152 * P] are sized for the worst case: a stream that takes fewer frames than the call, or
   that is mono in a P = 2 batch, still has a full row, and a host call copies all of it.  With segments in force the
   `pcm` / `d_pcm` argument of every encode and submit entry point of the batch is instead the base of one image of
   in_bytes bytes, and stream i's input is the len_i bytes at pcm + off[i], in the order its row would hold them:
     len_i = n_i * 1152 * ch_i * sample size, n_i = the frame count in force (hx_batch_frame_counts) or nframes,
     ch_i = hx_batch_stream_channels(b, i) as of the call, interleaved for a stereo stream.
   A kernel at the head of the call's front end (k_pcm_spread) copies the segments into a row buffer the batch owns
   (nstreams * nframes * 1152 * P samples of the call's type, made at the first call under segments), and the front end
   reads that: everything a call writes or leaves in the stream state is exactly what the same call writes when fed rows
   holding the same samples.  Device calls read the caller's image where it lies.
   hx_batch_pcm_segments: off is a HOST array [nstreams], copied by the function; NULL switches back to rows.  Returns
   0 / -1; sticky like hx_batch_frame_counts: a call takes the segments in force when it is made, and a submit's stay its
   own whatever is set afterwards.  It either sets the segments or (-1) changes nothing, and leaves the calling thread's
   current device alone.  Honoured by every encode and submit entry point of a plain batch: device and host buffers, s16
   and f32, *_stats, *_crc, *_host_dense, submit_*.  A converting batch returns -1: its input is per stream already.
   A call is refused (-1, hx_last_error names the stream) before anything is allocated, copied or launched, and the batch
   stays usable, unless for every stream with n_i > 0: off[i] >= 0, off[i] is a multiple of the call's sample size, and
   off[i] + len_i <= in_bytes.  off[i] of a stream with n_i = 0 is not looked at.
   Segments may leave gaps, come in any order and overlap (they are only read).  No 16-byte alignment is asked of the
   offsets or of a device image's base: a file's data chunk 44 bytes into a buffer is a valid segment start.
   Host calls copy one span of the image up: from the lowest segment start to the highest segment end among the streams
   that take frames.  Gaps inside the span cross the link with it, so a caller who wants minimal traffic packs tight:
   hx_pcm_packed_layout.  hx_batch_submit_*_host size their staging by the span.
   The offsets travel to the device through page-locked staging in rotation, as the counts do, with the same two notes:
   a call under segments may wait on the host for the upload of the third call before it, and it cannot be made while
   its stream is being captured into a graph.  Calls without segments do neither.
   hx_pcm_packed_layout: pure host code, no batch and no device.  The tight layout: off[0] = 0, off[i + 1] = off[i] + len_i
   with n_i = nfr ? nfr[i] : nframes and ch_i = channels[i]; sample_bytes is 2 or 4; off has nstreams + 1 entries.
   Returns off[nstreams], the image's size, or -1 for bad arguments: a null off or channels, a channel count other than 1
   or 2, a sample size other than 2 or 4, a count outside 0 .. nframes.  Every len_i is a multiple of 2304, so the tight
   layout is 16-byte aligned without padding.
   Not covered: converting batches, the hx_enc_* encoder, and bench.py, which measures calls fed rows. */
long long hx_pcm_packed_layout(int nstreams, int nframes, const int *nfr, const int *channels, int sample_bytes, long long *off);
int hx_batch_pcm_segments(hx_batch *b, const long long *off, long long in_bytes);
/* ---- PCM planes: a call's channel planes interleaved on the GPU (no reference equivalent) ----
   Every PCM entry point of a plain batch takes a stream's channels interleaved, floats at int16 scale.  A waveform tensor
   is channel-major ([streams, channels, time]) and usually fp32 in [-1, 1).  With planes in force the `pcm` / `d_pcm`
   argument of every encode and submit entry point of the batch is the base of one image of in_bytes bytes, and channel c
   of stream i is the n_i * 1152 consecutive samples at pcm + off[i] + c * chan_stride[i]:
     n_i = the frame count in force (hx_batch_frame_counts) or nframes, c < hx_batch_stream_channels(b, i) as of the call.
   A kernel at the head of the call's front end (k_pcm_planes, in k_pcm_spread's place) interleaves the planes into the row
   buffer the batch owns, and the front end reads that: everything a call writes or leaves in the stream state is exactly
   what the same call writes when fed rows holding the same samples.  Device calls read the caller's image where it lies.
   A sibling of PCM segments, with their contract wherever it is not restated here:
   hx_batch_pcm_planes: off and chan_stride are HOST arrays [nstreams], copied by the function.  A NULL chan_stride means
   the tight stride n_i * 1152 * sample size, formed per call; a NULL off switches back to rows.  Returns 0 / -1; sticky: a
   call takes the planes in force when it is made, and a submit's stay its own whatever is set afterwards.  It either sets
   the planes or (-1) changes nothing, and leaves the calling thread's current device alone.  Honoured by every encode and
   submit entry point of a plain batch: device and host buffers, s16 and f32, *_stats, *_crc, *_host_dense, *_host_files,
   *_host_recon, submit_*.  A converting batch returns -1.
   Segments and planes exclude each other: setting one replaces the other, and either setter with a NULL off goes back to
   rows.  A batch that never calls this setter behaves as before.
   chan_stride[i] may be any multiple of the call's sample size: [S, C, T] and [C, S, T] tensors, a negative stride, and 0,
   where both channels read one plane.  Planes may overlap between channels and between streams (they are only read).  A
   mono stream's stride is not looked at; neither are the offset and stride of a stream with n_i = 0.  No 16-byte alignment
   is asked of the offsets, the strides or a device image's base.
   unit_scale takes effect on fp32 calls only: 0 takes the samples as they are, at int16 scale; 1 takes every sample as
   x * 32768.0f, one IEEE float multiplication formed once in the interleaving kernel (subnormal inputs are kept, not
   flushed; an input beyond 2^113 gives an infinity).  Any other value is refused by the setter.  An s16 call made while
   unit_scale = 1 is in force is refused by name, not silently taken unscaled.
   A call is refused (-1, hx_last_error names stream and channel) before anything is allocated, copied or launched, and the
   batch stays usable, unless for every stream with n_i > 0 and each of its channels: the plane start is at or above 0, it
   is a multiple of the call's sample size, and the plane ends at or below in_bytes.
   Host calls copy one span of the image up: from the lowest plane start to the highest plane end among the streams that
   take frames.  hx_batch_submit_*_host size their staging by the span.
   Offsets and strides travel to the device as the segments' offsets do, in the same staging, with the same two notes.
   hx_pcm_planar_layout: pure host code.  The tight layout: a stream's planes back to back in channel order, the streams
   back to back in stream order: chan_stride[i] = n_i * 1152 * sample_bytes, off[0] = 0, off[i + 1] = off[i] + ch_i *
   chan_stride[i]; off has nstreams + 1 entries, chan_stride nstreams.  Returns the image's size, or -1 under
   hx_pcm_packed_layout's rules (and for a null chan_stride), writing nothing.  Every plane is a multiple of 2304 bytes, so
   the layout is 16-byte aligned.
   Not covered: converting batches, the hx_enc_* encoder, the command line, planar decoded PCM (hx_batch_recon_buffer
   keeps the rows' layout), and bench.py, which measures calls fed rows. */
long long hx_pcm_planar_layout(int nstreams, int nframes, const int *nfr, const int *channels, int sample_bytes, long long *off, long long *chan_stride);
int hx_batch_pcm_planes(hx_batch *b, const long long *off, const long long *chan_stride, long long in_bytes, int unit_scale);
/* ---- dense output: a call's bitstreams back to back (no reference equivalent) ----
   The rows [nstreams][out_stride] are sized for the worst case and mostly empty.  With dense output on, a call also
   gathers them on the GPU, behind its packing, into one image.  With nb[i] = out_bytes[i]:
     off[i] = sum over j < i of round_up(nb[j], 16), i = 0 .. nstreams; off[nstreams] is the image's size;
     dense[off[i] .. off[i] + nb[i]) = the first nb[i] bytes of row i; the bytes from there to off[i + 1] are zero.
   Every segment starts on a 16-byte boundary (at most 15 bytes of padding per stream and call); a stream that emitted
   nothing has an empty segment.  The rows and out_bytes are written as always: the image is in addition to them.
   If off[nstreams] > dense_cap, the offsets are still complete (the caller can size a retry), every segment that fits in
   whole (off[i + 1] <= dense_cap) is written, the others are not, nothing is written at or beyond dense + dense_cap, and
   status bit 16 is set (hx_batch_status).
   Not covered: hx_multi_* and the command-line tool's batch mode keep rows, and converting batches have no *_host_dense
   calls (their device call takes hx_batch_dense_buffers like any other). */
/* worst-case size of a call's dense image: nstreams * round_up(hx_batch_out_stride(b, nframes), 16) */
long long hx_batch_dense_bound(const hx_batch *b, int nframes);
/* optional dense output of the batched device calls; NULL switches it off.  d_dense: 16-byte aligned (else -1),
   d_dense_off: [nstreams + 1] long long.  Applies to the calls that follow; a call writes the buffers in force when
   it is made - a submit too: they travel with its deferred packing, must stay valid until the hx_batch_wait behind
   it, and consecutive submits take different sets (two in turn, like d_out). */
int hx_batch_dense_buffers(hx_batch *b, unsigned char *d_dense, long long dense_cap, long long *d_dense_off);
/* Host calls of which only the image crosses the link: dense [dense_cap] bytes, dense_off [nstreams + 1], out_bytes
   [nstreams]; the rows stay in the batch's device staging.  An image that does not fit still returns 0: the caller sees
   dense_off[nstreams] > dense_cap (and status bit 16), and has the segments that fit.  Synchronous calls: any host memory. */
int hx_batch_encode_s16_host_dense(hx_batch *b, const int16_t *pcm, int nframes, unsigned char *dense, long long dense_cap,
                                   long long *dense_off, int *out_bytes);
int hx_batch_encode_f32_host_dense(hx_batch *b, const float *pcm, int nframes, unsigned char *dense, long long dense_cap,
                                   long long *dense_off, int *out_bytes);
/* The pipelined form, completed by hx_batch_wait_host like hx_batch_submit_*_host (two sets of buffers in turn).  No copy
   brings the image down: the gather kernel stores it, and the offsets kernel dense_off, straight into the caller's memory,
   so dense (16-byte aligned) and dense_off must be page-locked (hx_pinned_alloc, or registered with the HIP runtime); with
   anything else the call is refused (-1, hx_last_error) before anything runs.  out_bytes travels by a small copy. */
int hx_batch_submit_s16_host_dense(hx_batch *b, const int16_t *pcm, int nframes, unsigned char *dense, long long dense_cap,
                                   long long *dense_off, int *out_bytes);
int hx_batch_submit_f32_host_dense(hx_batch *b, const float *pcm, int nframes, unsigned char *dense, long long dense_cap,
                                   long long *dense_off, int *out_bytes);
/* the settings an encoder would run a control with (what L3_audio_encode_info_ec / _info_head report,
   mp3enc.cpp:839-866), host only; 0 = configuration rejected */
int hx_control_info(const HX_E_CONTROL *ec, HX_E_CONTROL *ec_out, HX_MPEG_HEAD *head_out);
/* status bits accumulated by the kernels: 2 = main data overflow (the reference would assert
   there), 4 = the Huffman bits packed for a channel differ from the bits counted for it (an internal
   consistency check of the two-wave packer), 8 = a converter window out of bounds (converting batches), 16 = a dense image
   did not fit its dense_cap (hx_batch_dense_buffers; also the image of hx_batch_file_gather_device and its dst_cap), 32 = hx_batch_set_stream_states_device was handed a blob its slot does
   not take (that slot was left as it was), 64 = a file did not fit its image (hx_batch_file_images; the bytes that fit
   were written).  0 = healthy; -1 = no answer (the batch became unusable after a
   failed device call, or the status could not be read).  Synchronises - and, like hx_batch_wait, first enqueues the
   packing that the last hx_batch_submit_*_device left for later: that writes the submit's output buffers (d_out,
   d_out_bytes and the packet buffer that was set at the submit), which must therefore still be valid.
   hx_batch_gate_timeouts: how many pipelined submits started their front end late because the gate on the previous
   allocator launch gave up waiting (results are correct, overlap was lost; a loaded or profiled GPU can cause it).
   It is a performance counter, not part of the health status. */
int hx_batch_status(hx_batch *b);
int hx_batch_gate_timeouts(hx_batch *b);
/* Which build of the per-stream rate-loop kernel the batch runs (chosen at create from the batch size; the environment
   variable HMP3AMD_K6 = fat | slim overrides): 0 = k_alloc, four streams per CU, 1 = k_alloc_slim, six per CU.  Both
   restate the same reference code (bitallo3.cpp:484-3149) and produce the same bytes.  hx_batch_resident_streams: how many
   of the batch's streams the device holds at once with that kernel. */
int hx_batch_k6_variant(const hx_batch *b);
int hx_batch_resident_streams(const hx_batch *b);
/* identifies the build: a hash of the library's sources and code-generation flags (hmp3_amd/build.sh) */
const char *hx_build_id(void);
/* total frames / bytes emitted so far by stream i (synchronises) */
HX_INT_PAIR hx_batch_frames_bytes(hx_batch *b, int stream_index);
/* mean device time of the dominant (allocator) kernel over the calls since the last query, in
   milliseconds, measured with HIP events on the launch stream; also returns the call count */
float hx_batch_alloc_kernel_ms(hx_batch *b, int *ncalls);

/* ---- converting batches: sources in any format and at any rate the converter takes, converted on the GPU ----
   Per stream, ec is the control CMp3Enc::MP3_audio_encode_init takes (samprate = the source's rate, mode 3 = a mono
   source) and src its other arguments; the streams' resolved encode controls follow hx_batch_create's rules (one channel
   count, MPEG-1 or MPEG-2 rates, first-generation allocator or not).  A source the converter rejects makes create return
   NULL, with the stream named in hx_last_error.  Each call of nframes frames is nframes calls of
   CMp3Enc::MP3_audio_encode per stream: the converter (k_src) writes the fp32 PCM the encoder reads, bit-identical to
   hx_src_convert, and everything behind it is the fp32 path (DC filter, packets, frame counters, taps included).
   The other hx_batch_* calls apply; hx_batch_reset_stream also restarts the stream's converter, and the stream-state blob
   of a converting batch also holds the converter's phase and carried samples (it is larger, and refused by a batch of
   the other kind).  hx_batch_debug_read(b, "srcpcm", ...): the converted PCM of the last call, [S][nframes*1152][nch].
   A converting batch refuses the int16 / fp32 encode and submit calls (-1): they would advance the encoder past its
   converter.  Status bit 8 (hx_batch_status): a call's window exceeded the converter plan's bound (cannot happen; the
   call's converted PCM was not written). */
hx_batch *hx_batch_create_src(int device, int nstreams, const HX_E_CONTROL *ec, int shared_control, const HX_SOURCE *src,
                              int shared_source, int max_frames);
/* host only, changes nothing: the bytes each of stream i's next nframes calls consumes (in_bytes may be NULL); returns the
   bytes those calls read, counted from the stream's first unconsumed byte */
long long hx_batch_src_schedule(const hx_batch *b, int i, int nframes, long long *in_bytes);
/* an in_stride that fits nframes consecutive calls of every stream, from the rates alone */
long long hx_batch_src_in_stride(const hx_batch *b, int nframes);
/* in: [nstreams][in_stride] bytes, row i starting at stream i's first unconsumed byte.  frame_off (host): NULL, or
   [nstreams][nframes] byte offsets into the row where call f's input starts (the reference takes a pointer per call);
   NULL = each call starts where the previous one's consumption ended.  in_used (host, [nstreams], may be NULL): where a
   following call would start, known when the function returns.  A row shorter than its schedule or an offset that
   reads past in_stride is refused before anything runs (-1, the batch stays usable).  Asynchronous on `stream`. */
int hx_batch_encode_src_device(hx_batch *b, const unsigned char *d_in, long long in_stride, const long long *frame_off,
                               int nframes, unsigned char *d_out, long long out_stride, int *d_out_bytes,
                               long long *in_used, void *stream);
/* the same with host buffers (synchronous); stats: NULL or [nstreams][nframes][2], as hx_batch_encode_f32_host_stats */
int hx_batch_encode_src_host(hx_batch *b, const unsigned char *in, long long in_stride, const long long *frame_off,
                             int nframes, unsigned char *out, long long out_stride, int *out_bytes,
                             long long *in_used, int *stats);
/* ---- converting calls under per-stream frame counts: the counts come with the call, like frame_off and in_used ----
   nfr: HOST array [nstreams], copied by the call; NULL = every stream takes nframes, which is exactly
   hx_batch_encode_src_device / _host.  stats: NULL or [nstreams][nframes][2]; crc: NULL or [nstreams][nframes], the
   per-frame MusicCRC as hx_batch_encode_f32_host_crc returns it; crc without stats is refused (-1) before anything runs.
   With n = nfr[i]:
     - refusals: a call with any n < 0 or n > nframes returns -1 before anything is allocated, copied, launched or
       counted, and hx_last_error names the stream (hx_multi: by its number over all blocks, and no block starts).  After
       a refusal the batch stays usable and hx_batch_src_schedule answers as before the call;
     - input: stream i's row must hold the input of its first n calls - the extent check uses n, not nframes: without
       frame_off the closed form at the stream's call c0 + n - 1, with frame_off the entries f < n only (entries f >= n may
       hold anything, they are neither read nor checked).  n = 0: nothing of row i and none of its offsets is read.  Row
       bytes beyond what those n calls read have no influence on any output or state;
     - converter: the stream's converter advances n calls; in_used[i] is where call n would start (n = 0: 0); the
       "srcpcm" tap holds frames f < n, the rest of the stream's row there is not written;
     - n = 0: the converter's call count and its carried samples are unchanged, the stream's checkpoint
       (hx_batch_get_stream_state, converter part included) is bit-identical before and after, out_bytes[i] = 0 and row i
       is not written;
     - rows, out_bytes, frame counters, packet sizes, MusicCRC, the dense image and the encoder state follow the rules of
       hx_batch_frame_counts word for word: per stream it is the reference's MP3_audio_encode called n times.
   The restrictions of plain calls under counts apply (three page-locked copies in rotation: the call may wait on the
   host for the upload of the third call before it, and cannot be captured into a graph); calls with nfr = NULL have
   neither.
   Not covered: pipelined submits of converting batches, and *_host_dense calls for them. */
int hx_batch_encode_src_counts_device(hx_batch *b, const unsigned char *d_in, long long in_stride, const long long *frame_off,
                                      int nframes, const int *nfr, unsigned char *d_out, long long out_stride, int *d_out_bytes,
                                      long long *in_used, void *stream);
int hx_batch_encode_src_counts_host(hx_batch *b, const unsigned char *in, long long in_stride, const long long *frame_off,
                                    int nframes, const int *nfr, unsigned char *out, long long out_stride, int *out_bytes,
                                    long long *in_used, int *stats, unsigned short *crc);

/* ---- file ledger: where each stream's file ends, its MusicCRC and its seek points, kept on the GPU (no reference
   equivalent; per file it is what the single-file loop of tomp3.cpp:976-1036 keeps on the host) ----
   A caller that runs files through a batch has to decide, per file, at which frame the file's drain ends
   ("while (get_frames() < frames_expected)"), which bytes of the call that holds this frame belong to the file, the
   MusicCRC of those bytes, and the seek points of the Xing tag (one hx_xing_toc per input call).  From the frame counters
   and CRCs that is one host iteration per encoded frame.  A ledger does it on the device: one HX_LEDGER record per
   stream, updated by a kernel right behind a call's CRC kernel, read when convenient.
   The record (fixed layout, sizeof a multiple of 16, padding words always 0: two records compare bytewise): */
#define HX_LEDGER_POINTS 513    /* xhead.c:71 keeps 512 seek points; XingHeaderUpdateInfo appends the file's end */
typedef struct {
    /* the file's parameters (hx_ledger_open) */
    int ncalls;                 /* >= 1: the calls of the single-file loop on the file's input */
    int frames_per_call;        /* 1, or 2 at the MPEG-2 rates */
    int head_bytes;             /* the tag frame's size, 0 without a tag */
    int flags;                  /* bit 0: keep seek points */
    /* the state; expected = ncalls * frames_per_call */
    int open, ended;
    int fed;                    /* calls consumed so far */
    unsigned frames, bytes;     /* the file's get_frames() and bytes so far; final once ended */
    unsigned crc;               /* the MusicCRC of those bytes (16 bits) */
    int call_bytes;             /* how many bytes of the row of the last call that fed it belong to the file */
    int toc_counter, npt, every;                /* the seek-point state of hx_xing: calls to the next point, points held, */
    int pad0[2];                                /* and the spacing of the points in calls */
    int pt[HX_LEDGER_POINTS][2];                /* (frames, bytes) */
    int pad1[2];
} HX_LEDGER;
/* A call updates stream i's record as follows.  The stream takes n frames (its per-stream count, or nframes);
   (fr[f], by[f]) are its frame counters, c[f] its per-frame CRCs, nb = out_bytes[i], e[f] as under hx_batch_crc_buffer:
     not open, or n == 0:   the record is bit-identical before and after
     ended:                 call_bytes = 0, nothing else changes (the slot may go on encoding silence; it no longer counts)
     otherwise, for f = 0 .. n-1, with u = fed + f:
         if u < ncalls and (flags & 1):  if (--toc_counter <= 0) toc_counter = toc_step(fr[f] + 1, by[f] + head_bytes)
         if u >= ncalls - 1 and (unsigned) fr[f] >= expected:     the drain ends here:
             frames = fr[f]; bytes = by[f]; crc = combine(crc, c[f], e[f]); call_bytes = e[f]; fed = u + 1; ended = 1; stop
     not ended after f = n-1:
         frames = fr[n-1]; bytes = by[n-1]; crc = combine(crc, c[n-1], nb); call_bytes = nb; fed += n
   toc_step is hx_xing_toc (append; at 512 points keep every second one and double `every`), combine is
   hx_xing_crc_combine.
   Host side, no GPU: hx_ledger_open fills a new record; hx_ledger_update applies the rule to one stream's slice of one
   call (stats [n][2], crc [n]; returns 1 when the call ended the file) - for callers that keep their counters on the host
   and for the hx_enc_* route; hx_xing_load_points copies a record's seek points into an hx_xing, after which
   hx_xing_update_info(..., toc = NULL, ...) builds the 100 TOC bytes as after the hx_xing_toc calls themselves (1 = ok,
   0 = a record whose point count is out of range). */
void hx_ledger_open(HX_LEDGER *r, int ncalls, int frames_per_call, int head_bytes, int flags);
int hx_ledger_update(HX_LEDGER *r, const int *stats, const unsigned short *crc, int n, int out_bytes);
/* The batch's records: [nstreams] on the device, allocated and zeroed (all closed) at the first hx_batch_ledger_begin; a
   batch that never calls it allocates nothing and launches nothing more than before.
   hx_batch_ledger_begin: slot idx[e] gets a new open record with open[e]'s ncalls, head_bytes and flags (reserved: 0) and
   the batch's frames_per_call.  A slot operation with hx_batch_reset_streams' contract word for word: a HOST list of
   distinct slots, one launch whatever n is, ordered like a plain device call behind everything the batch has in flight
   (the deferred packing of the last submit goes out first, ungated, so the previous occupant's last update is through),
   the list through the slot operations' staging rotation, not under stream capture, n = 0 returns 0 and launches nothing,
   the same refusals before anything is allocated, uploaded or launched, plus a null `open` with n > 0 and
   "entry e: ncalls < 1" / "entry e: head_bytes < 0".  It does not reset the encoder: pair it with hx_batch_reset_streams
   or hx_batch_assign_streams, in either order (the second of the two finds nothing deferred).  The counters a ledger reads
   are the stream's absolute get_frames() and bytes, so a record is meaningful only for a stream that was reset (or new)
   when its file began.
   Calls while the ledger exists: the update kernel goes out right behind the call's CRC kernel - of a submit with its
   deferred packing, reading the counters, CRCs, byte counts and per-stream counts of its own submit; deferred packings go
   out in submit order on one stream, so the records advance in call order.  Every encode or submit entry point, plain
   and converting, device and host buffers, whose call feeds (n > 0) at least one record that is open and not known to have
   ended needs a frame-counter buffer and a CRC buffer in force (host calls: the forms that return both, *_host_crc and
   hx_batch_encode_src_counts_host with stats and crc); otherwise the call is refused (-1, hx_last_error names the stream)
   before anything runs and the batch stays usable.  "Known to have ended": the end is decided on the device, and the host
   learns it from hx_batch_ledger_read; until a read has shown a record ended, it counts as live.  Rows, out_bytes, packets,
   counters, CRCs and the dense image are written exactly as without a ledger; the dense image follows out_bytes, not
   call_bytes.
   hx_batch_ledger_read: record e of out[n] is slot idx[e]'s.  Synchronous like hx_batch_status: enqueues the deferred
   packing first, then one gather launch and one copy whatever n is.  hx_batch_ledger_read_device: the same gather in
   stream order into device memory (16-byte aligned, else -1), like hx_batch_get_stream_states_device; it does not tell the
   host which records ended.
   hx_multi_ledger_begin / hx_multi_ledger_read: the same over all blocks (idx counts streams over all blocks); synchronous,
   every refusal made for all blocks before one of them starts: all blocks or (-1) none.
   Not covered: the checkpoint blob (state version 3, no ledger in it) - a stream moved between batches takes its record
   along through hx_batch_ledger_read and a new hx_batch_ledger_begin, which restarts it; moving a half-built record; the
   hx_enc_* encoder, which has hx_ledger_update on the host. */
typedef struct { int ncalls, head_bytes, flags, reserved; } HX_LEDGER_OPEN;
int hx_batch_ledger_begin(hx_batch *b, const int *idx, const HX_LEDGER_OPEN *open, int n, void *stream);
int hx_batch_ledger_read(hx_batch *b, const int *idx, int n, HX_LEDGER *out);
int hx_batch_ledger_read_device(hx_batch *b, const int *idx, int n, HX_LEDGER *d_out, void *stream);

/* ---- file images: each file's bitstream gathered on the GPU, fetched once (no reference equivalent) ----
   The ledger decides on the device which bytes of a call belong to a file (call_bytes).  With file images on, a kernel
   right behind the ledger's update also puts those bytes where the file is: every slot owns an image of `cap` bytes of
   device memory (16-byte aligned start), of which
     bytes [0, head_bytes) are reserved for the tag frame - only k_file_tag writes them, when asked (hx_batch_file_tags,
     "finished files" below);
     the file's audio bytes follow from head_bytes, contiguous, in call order.
   Per slot the batch keeps one length word beside the ledger, image_bytes: the audio bytes present in the image.  It equals
   the record's `bytes`, or less after an overflow.  HX_LEDGER and the checkpoint blob are as before.
   A call appends for stream i when the stream takes n > 0 frames of it, its record is open, and the record was begun while
   images were on: the call_bytes bytes at the start of row i go to image_i + head_bytes + (bytes - call_bytes), bytes and
   call_bytes as the call's ledger update left them.  A stream that takes no frames, a record that is not open and a record
   that had already ended keep image and length word bit-identical.  Nothing at or beyond cap is written: of a file that
   does not fit, the bytes that fit are written, image_bytes stops at cap - head_bytes and status bit 64 is set
   (hx_batch_status); the other streams are unaffected and the batch stays usable.
   Composition: every encode or submit entry point of a batch with images on appends - device and host buffers, plain and
   converting, a submit with its deferred packing - under the ledger's own rule (the call has a frame-counter and a CRC buffer
   in force).  Rows, out_bytes, packets, counters, CRCs, the dense image and the ledger records are written exactly as
   without images, and a batch that never switches images on allocates and launches nothing more than before.
   hx_batch_file_images: switches images on with cap > 0 (allocates nstreams * round_up(cap, 16) bytes; an earlier set of
   images is released) or off with cap = 0.  Synchronous; sticky.  Refused (-1, nothing changes) while the host counts any
   record as live (begun, and not shown ended by hx_batch_ledger_read or hx_batch_ledger_poll), for a negative cap, and when
   the allocation fails - the batch stays usable, and the earlier images and their cap stay in force: the new set is
   allocated before the old one is released, so a change of cap needs room for both for a moment (switch off first where
   that is too much).  Records begun before it was called have no image (image_bytes stays 0); it sets every length word
   to 0.
   hx_batch_ledger_begin sets image_bytes to 0 for the slots it opens; it does not clear the image, so the previous file's
   bytes stay until overwritten.  Reset, assign, save and restore do not touch images.
   hx_batch_file_image_cap: cap, 0 = off.  hx_batch_file_image_ptr: the device address of slot i's image (NULL: off, or i
   out of range), for device consumers and tests.
   The short form of a record (fixed layout, 32 bytes, two of them compare bytewise): */
typedef struct { int open, ended, fed; unsigned frames, bytes, crc; int call_bytes; unsigned image_bytes; } HX_LEDGER_BRIEF;
/* hx_ledger_brief: host only, the reference for the kernel: the record's fields of the same names, and image_bytes as given.
   hx_batch_ledger_poll: out [nstreams], the brief of every slot's record (all zero but image_bytes for a batch without a
   ledger).  Synchronous like hx_batch_ledger_read: the deferred packing first, then one launch and one copy of
   32 * nstreams bytes.  It teaches the host which records have ended, exactly as a read does.
   hx_batch_ledger_poll_device: the same launch in stream order into device memory, d_out [nstreams], 16-byte aligned (else
   -1); it does not inform the host.
   hx_batch_file_fetch: synchronous.  Copies the image_bytes audio bytes of slot i to dst + head_bytes (head_bytes: of the
   slot's latest hx_batch_ledger_begin), leaves dst[0, head_bytes) untouched for the caller's tag frame, and returns
   head_bytes + image_bytes - or -1 without copying if that exceeds dst_cap, if images are off, or for a bad argument.
   Works for live and ended records alike.
   Host-fed calls that bring nothing down but the call's status: hx_batch_encode_{s16,f32}_host_files and, for converting
   batches, hx_batch_encode_src_files_host (nfr: HOST [nstreams] or NULL, in_used: [nstreams] or NULL, as
   hx_batch_encode_src_counts_host).  Rows, byte counts, frame counters and CRCs live in staging the batch owns on the
   device; the ledger and the images advance.  They honour hx_batch_frame_counts and hx_batch_pcm_segments like every other
   host call, and are refused (-1, before anything runs) when the batch has no ledger or no images.  They return the status
   bits as hx_batch_status would after the call (0 = healthy; bit 64 = a file did not fit), or -1.
   hx_multi_file_images / hx_multi_ledger_poll / hx_multi_file_fetch (i counts streams over all blocks) /
   hx_multi_encode_{s16,f32}_host_files / hx_multi_encode_src_files_host: the same over all blocks, under the hx_multi rules:
   all blocks or (-1) none, refusals made for all blocks before one starts, the caller's stream numbers in messages; the
   encode calls return the blocks' status bits or'ed.  (hx_multi_file_images: a block whose allocation fails after another's
   succeeded has that one's images released again.)
   Not covered: images in the checkpoint blob - a stream moved between batches leaves its image behind; pipelined host
   submits in a _files form; the hx_enc_* encoder; bench.py, which measures calls that return rows.

   ---- finished files: the tag frame built on the GPU, many files fetched at once ----
   The tag's description: what the command-line tool's Tagger passes to hx_xing_header and hx_xing_update_info that the
   record does not hold (fixed layout, 48 bytes, reserved: 0). */
typedef struct { int samprate, h_mode, cr_bit, original_bit, flags, kbps, vbr_scale;   /* hx_xing_header's arguments; vbr_scale -1 = CBR */
                 unsigned lowpass, in_samplerate, reserved;                             /* hx_xing_update_info's; out_samplerate = samprate */
                 unsigned long long samples_audio; } HX_FILE_TAG;
/* hx_file_tag_bytes: host only; the tag frame's size, what hx_xing_header returns for these arguments (0 = no tag, or it
   does not fit the frame) - the head_bytes to give hx_batch_ledger_begin.
   hx_file_tag_build: host only, pure, the reference for the kernel.  Writes into buf [cap] exactly the bytes that
     hx_xing_header(x, samprate .. flags, frames 0, bytes 0, vbr_scale, toc NULL, buf, NULL, NULL, kbps);
     hx_xing_load_points(x, r);
     hx_xing_update_info(x, r->frames, n, vbr_scale, NULL, buf, NULL, NULL, samples_audio, n, lowpass, in_samplerate, samprate, r->crc)
   leave in the first head_bytes bytes, with n = r->head_bytes + r->bytes, on a seek table of its own: *r is not changed
   (the TOC's end point and scaling go into a copy).  Returns the size, or 0 - nothing written - when
   hx_file_tag_bytes(t) != r->head_bytes, when that is 0 or exceeds cap, or when the record's point state is out of range.
   hx_batch_file_tags: after it, bytes [0, head_bytes) of slot idx[e]'s image equal hx_file_tag_build(record, &tags[e]) byte
   for byte - of a live record the tag of the state so far, of an ended one the file's.  A slot operation with
   hx_batch_ledger_begin's contract word for word: a HOST list of distinct slots, one launch whatever n is (k_file_tag, one
   workgroup per listed slot), ordered behind everything the batch has in flight (the deferred packing first), the entries
   through the slot operations' staging rotation, not under stream capture, n = 0 returns 0 and launches nothing.  Refused
   before anything is uploaded or launched, with the entry named: images off; a slot whose record was not begun with an
   image; a null `tags` with n > 0; hx_file_tag_bytes(&tags[e]) differing from the head_bytes of the slot's latest begin.
   A slot with head_bytes 0 is accepted and nothing is written for it.  Idempotent: a second call with other parameters
   rebuilds the whole head.  It writes nothing at or beyond head_bytes and leaves the record, the length word and every other
   slot's image bit-identical.  (A record whose point state is out of range, or whose head_bytes on the device is not the
   tag's size or exceeds cap, gets nothing written - where the host function returns 0.)
   The fetch of many files: the layout is the dense image's.  Segment e is slot idx[e]'s head_bytes + image_bytes bytes from
   the start of its image - head room included, so behind hx_batch_file_tags a complete file - at
     off[e] = sum over j < e of round_up(len_j, 16), e = 0 .. n; off[n] is the total;
   the bytes from the segment's end to off[e + 1] are zero.  Segments come in list order; any order and any subset of
   distinct slots.  The lengths are the device's own words (the record's head_bytes, the slot's image_bytes; never more than
   cap), so a live record's segment is what the device holds at that point of the stream order.
   hx_batch_file_gather_device: in stream order like hx_batch_ledger_poll_device, behind everything in flight: k_file_off
   (the scan, into d_off [n + 1]) and k_file_gather (into d_dst), the list through the slot operations' staging; d_dst 16-byte
   and d_off 8-byte aligned, else -1; not under stream capture.  The offsets are always complete; a segment that does not
   fit dst_cap in whole (off[e + 1] > dst_cap) is not written, nothing at or beyond d_dst + dst_cap is, and status bit 16 is set.
   hx_batch_file_fetch_many: synchronous, behind a drain: the scan, a copy of the offsets into off [n + 1], refusal (-1, dst
   untouched, off filled) when off[n] > dst_cap, the gather into device staging that the batch owns (grown to the largest
   total so far, released with the images), one copy of off[n] bytes: two launches and two copies whatever n is.  Returns
   off[n].  Sets no status bit.
   Both refuse (-1) images off, a null idx / off / dst with n > 0 and the slot operations' list errors; n = 0 returns 0,
   launches nothing and writes off[0] = 0 where off is given (the device form: nothing).
   hx_multi_file_tags / hx_multi_file_fetch_many: the same over all blocks (idx counts streams over all blocks); synchronous;
   refusals made for all blocks before one starts; the result is what the one-batch call would give for the list: segments
   in the caller's order, one off array.
   Not covered: a _files form of the pipelined host submits; images in the checkpoint blob; the hx_enc_* encoder; a gather
   straight into the caller's page-locked memory (the host form goes through device staging and one copy). */
int hx_file_tag_bytes(const HX_FILE_TAG *t);
int hx_file_tag_build(const HX_LEDGER *r, const HX_FILE_TAG *t, unsigned char *buf, int cap);
int hx_batch_file_tags(hx_batch *b, const int *idx, const HX_FILE_TAG *tags, int n, void *stream);
long long hx_batch_file_fetch_many(hx_batch *b, const int *idx, int n, unsigned char *dst, long long dst_cap, long long *off);
int hx_batch_file_gather_device(hx_batch *b, const int *idx, int n, unsigned char *d_dst, long long dst_cap, long long *d_off, void *stream);
void hx_ledger_brief(const HX_LEDGER *r, unsigned image_bytes, HX_LEDGER_BRIEF *out);
int hx_batch_file_images(hx_batch *b, long long cap);
long long hx_batch_file_image_cap(const hx_batch *b);
unsigned char *hx_batch_file_image_ptr(hx_batch *b, int i);
int hx_batch_ledger_poll(hx_batch *b, HX_LEDGER_BRIEF *out);
int hx_batch_ledger_poll_device(hx_batch *b, HX_LEDGER_BRIEF *d_out, void *stream);
long long hx_batch_file_fetch(hx_batch *b, int i, unsigned char *dst, long long dst_cap);
int hx_batch_encode_s16_host_files(hx_batch *b, const int16_t *pcm, int nframes);
int hx_batch_encode_f32_host_files(hx_batch *b, const float *pcm, int nframes);
int hx_batch_encode_src_files_host(hx_batch *b, const unsigned char *in, long long in_stride, const long long *frame_off,
                                   int nframes, const int *nfr, long long *in_used);

/* ---- host placement (no reference equivalent): a host-fed GPU reads ~50 GB/s of PCM over PCIe, so its page-locked
   buffers and the threads that submit its copies belong on the NUMA node the device hangs on.
   hx_device_numa_node: that node from sysfs (-1 = unknown or not a NUMA machine).  hx_bind_thread_to_device: restricts the
   calling thread to the CPUs of that node which the process may use and returns their number (0 = nothing changed); call it
   before hx_pinned_alloc so that first touch places the pages there.  hx_multi_* binds its per-device threads itself.
   "The CPUs the process may use" are the ones its loading thread had when the library was loaded: a thread bound to one
   device's node can be bound to another device's node afterwards.  hx_bind_thread_to_node: the same by node number. */
int hx_device_numa_node(int device);
int hx_bind_thread_to_device(int device);
int hx_bind_thread_to_node(int node);
/* The process's CPU set is captured when the library is loaded.  A process that is narrowed or moved afterwards (taskset -p,
   os.sched_setaffinity by a launcher, a cpuset change) calls this from any thread to take the set again from its main
   thread's current mask; returns the number of CPUs (0 = failed, nothing changed).  The bind calls retry with it once by
   themselves when the kernel rejects the mask they computed from the stale set. */
int hx_refresh_process_cpus(void);

/* ---- several GPUs of one node behind one handle (no reference equivalent) ----
   nstreams independent streams in contiguous blocks over ndev devices (devices[0..ndev), or devices
   0..ndev-1 when devices is NULL; ndev <= 0: every device present), block sizes differing by at most one;
   one hx_batch per device, one host thread per device and call, nothing exchanged between devices.
   Buffers as in the hx_batch_*_host calls, covering all nstreams streams; out_stride >= hx_multi_out_stride. */
typedef struct hx_multi hx_multi;
hx_multi *hx_multi_create(int ndev, const int *devices, int nstreams, const HX_E_CONTROL *ec, int shared_control, int max_frames);
void hx_multi_destroy(hx_multi *m);
int hx_multi_ndevices(const hx_multi *m);
int hx_multi_nstreams(const hx_multi *m);
int hx_multi_shard(const hx_multi *m, int k, int *device, int *first, int *count);   /* block k: its device and streams */
hx_batch *hx_multi_batch(hx_multi *m, int k);                                        /* block k's batch, for the per-batch calls */
long long hx_multi_out_stride(const hx_multi *m, int nframes);
int hx_multi_encode_s16_host(hx_multi *m, const int16_t *pcm, int nframes, unsigned char *out, long long out_stride, int *out_bytes);
int hx_multi_encode_f32_host(hx_multi *m, const float *pcm, int nframes, unsigned char *out, long long out_stride, int *out_bytes);
int hx_multi_encode_f32_host_stats(hx_multi *m, const float *pcm, int nframes, unsigned char *out, long long out_stride, int *out_bytes, int *stats);
/* hx_batch_encode_f32_host_crc over all streams: stats [nstreams][nframes][2] and crc [nstreams][nframes], both required */
int hx_multi_encode_f32_host_crc(hx_multi *m, const float *pcm, int nframes, unsigned char *out, long long out_stride, int *out_bytes, int *stats,
                                 unsigned short *crc);
/* [nstreams] over all blocks; fanned out to the blocks' batches, all of them or (-1) none.  A call whose counts do not fit
   its nframes is refused for all blocks before any of them starts, and hx_last_error names the stream by its number here */
int hx_multi_frame_counts(hx_multi *m, const int *nfr);
/* hx_batch_pcm_segments over all blocks ("PCM segments" above): off [nstreams] addresses the caller's ONE image of in_bytes
   bytes, whose base every hx_multi_encode_*_host* call then takes as pcm; each block copies only its own streams' span.
   All blocks or (-1) none.  A call's segment checks run for all blocks, with the caller's stream numbers, before any block starts */
int hx_multi_pcm_segments(hx_multi *m, const long long *off, long long in_bytes);
/* hx_batch_pcm_planes over all blocks ("PCM planes" above), the same way: off and chan_stride [nstreams] address the caller's
   one image, and a call is checked for all blocks, with the caller's stream numbers, before one block starts. */
int hx_multi_pcm_planes(hx_multi *m, const long long *off, const long long *chan_stride, long long in_bytes, int unit_scale);
int hx_multi_status(hx_multi *m);
/* converting batches (hx_batch_create_src) in the same blocks: in [nstreams][in_stride], frame_off [nstreams][nframes] or NULL,
   in_used [nstreams], stats NULL or [nstreams][nframes][2], all as in hx_batch_encode_src_host over all streams */
hx_multi *hx_multi_create_src(int ndev, const int *devices, int nstreams, const HX_E_CONTROL *ec, int shared_control,
                              const HX_SOURCE *src, int shared_source, int max_frames);
/* hx_batch_create_menu in the same blocks: every block's batch gets the whole menu, cfg [nstreams] over all blocks or NULL */
hx_multi *hx_multi_create_menu(int ndev, const int *devices, int nstreams, const HX_E_CONTROL *ec, int nmenu,
                               const HX_SOURCE *src, const int *cfg, int max_frames);
/* the same over all blocks (idx counts streams over all blocks); synchronous like the other hx_multi calls; all blocks or (-1) none */
int hx_multi_assign_streams(hx_multi *m, const int *idx, const int *cfg, int n);
/* hx_batch_create_any in blocks over several devices ("one batch for every stream kind" above) */
hx_multi *hx_multi_create_any(int ndev, const int *devices, int nstreams, const HX_E_CONTROL *ec, int nmenu,
                              const HX_SOURCE *src, const int *cfg, int max_frames);
/* hx_batch_create_mixed in blocks over several devices ("mixed batches" above) */
hx_multi *hx_multi_create_mixed(int ndev, const int *devices, int nstreams, const HX_E_CONTROL *ec, int nmenu,
                                const HX_SOURCE *src, const int *cfg, int max_frames);
/* hx_batch_ledger_begin / hx_batch_ledger_read over all blocks (idx counts streams over all blocks); synchronous; all blocks or (-1) none */
int hx_multi_ledger_begin(hx_multi *m, const int *idx, const HX_LEDGER_OPEN *open, int n);
int hx_multi_ledger_read(hx_multi *m, const int *idx, int n, HX_LEDGER *out);
/* file images over all blocks ("file images" above): cap is per stream; out [nstreams]; i counts streams over all blocks */
int hx_multi_file_images(hx_multi *m, long long cap);
int hx_multi_ledger_poll(hx_multi *m, HX_LEDGER_BRIEF *out);
long long hx_multi_file_fetch(hx_multi *m, int i, unsigned char *dst, long long dst_cap);
/* hx_batch_file_tags / hx_batch_file_fetch_many over all blocks ("finished files" above) */
int hx_multi_file_tags(hx_multi *m, const int *idx, const HX_FILE_TAG *tags, int n);
long long hx_multi_file_fetch_many(hx_multi *m, const int *idx, int n, unsigned char *dst, long long dst_cap, long long *off);
int hx_multi_encode_s16_host_files(hx_multi *m, const int16_t *pcm, int nframes);
int hx_multi_encode_f32_host_files(hx_multi *m, const float *pcm, int nframes);
int hx_multi_encode_src_files_host(hx_multi *m, const unsigned char *in, long long in_stride, const long long *frame_off, int nframes,
                                   const int *nfr, long long *in_used);
long long hx_multi_src_in_stride(const hx_multi *m, int nframes);
int hx_multi_encode_src_host(hx_multi *m, const unsigned char *in, long long in_stride, const long long *frame_off, int nframes,
                             unsigned char *out, long long out_stride, int *out_bytes, long long *in_used, int *stats);
/* hx_batch_encode_src_counts_host over all streams: nfr [nstreams] or NULL, crc NULL or [nstreams][nframes] (needs stats).
   A count out of range or a row too short for its stream's calls refuses the call for all blocks before any of them starts */
int hx_multi_encode_src_counts_host(hx_multi *m, const unsigned char *in, long long in_stride, const long long *frame_off, int nframes,
                                    const int *nfr, unsigned char *out, long long out_stride, int *out_bytes, long long *in_used,
                                    int *stats, unsigned short *crc);

/* ---- test taps (tests only; synchronise) ---- */
/* name: "sb" "xr" "etab" "thr" "msbase" "bt" "eng" "dbg" (per-stage buffers), "ixq" "sgn" "seg" "frm" (what the allocator hands the
   packer), "dur" (per-stream duration of the last allocator launch, 100 MHz ticks), "place" (where position i of that launch's
   order ran: XCC id << 16 | HW_ID[15:0], i.e. CU [11:8], SH [12], SE [15:13]), "state", and two device counters (one int
   each, running over the batch's calls): "big_sweeps" = noise passes that took the double-precision x^(4/3) table,
   "strict_sums" = certified band sums that fell back to the reference's strict line-order sum (DESIGN.md section 2;
   HMP3AMD_EXACT_SUMS=1 sends every sum there), and "pcmrows" (the row buffer as the last call under PCM segments or PCM planes left it,
   [nstreams][that call's nframes * 1152 * P] samples of its type; -1 before the first such call).  Copies at most cap
   bytes, returns bytes, -1 for an unknown name. */
long long hx_batch_debug_read(hx_batch *b, const char *name, void *dst, long long cap);
/* Test tap: the head of a call's front end alone.  With PCM segments or PCM planes in force, makes a plain device call's
   checks of d_pcm (the image's base in device memory; f32: 0 = int16, 1 = fp32) and nframes, uploads the image's layout
   and launches the row kernel (k_pcm_spread / k_pcm_planes) on `stream` - and nothing behind it: no stream of the batch
   moves, no output is written.  The rows are then read with hx_batch_debug_read's "pcmrows" tap.  This is how the row
   kernels are held on samples the encoder behind them is not defined for (an fp32 product that overflows to an infinity).
   Returns 0 / -1 with hx_last_error; -1 without segments or planes in force, and on a converting batch. */
int hx_batch_debug_pcm_rows(hx_batch *b, const void *d_pcm, int nframes, int f32, void *stream);
void hx_batch_debug_enable(hx_batch *b, int on);
/* The kernels' device math on arguments of the caller's: for each i < n the device evaluates the function `name` - the
   very function the kernels call, built with the allocator kernels' flags, on this batch's device tables (the class-
   independent ones and those of the batch's first class) - on in[i] and stores out[i].  Everything crosses as 32-bit
   patterns, nothing is converted: floats as their bits, ints as int32.  A function of k operands reads in as [k][n].
     "logf" "log10f"            the restated logf and log10f of hmp3_amd/csrc/hx_libm32.h                   f32 -> f32
     "a1_mask_db"               (float) (-10.0 * (double) log10f r - (double) cbw), that log10f        (r, cbw) -> f32
     "a1_gz"                    (int) (a1_gz1 * logf m + a1_gz2), that logf, the class's constants          f32 -> i32
     "dblog"                    (float) (10.0 * log10((double) x)), the device's double log10               f32 -> f32
     "dual_g"                   (int) (1.7717f * dblog(x) + 1.0f), trade_dual's gain step                   f32 -> i32
     "is_scale" "is_scale_lsf"  the intensity bands' rescale before its clamp, MPEG-1 / MPEG-2       (e0, e1, r) -> f32
     "div"                      a / b in fp32                                                            (a, b) -> f32
     "mblog" "mblog16"          the millibel log, on the int table and on its 16-bit form                   f32 -> i32
     "mbexp"                    its inverse                                                                 i32 -> f32
     "pow34"                    x^(3/4), the piecewise-linear fit                                           f32 -> f32
     "round"                    (int) (x + copysign(0.5, x))                                                f32 -> i32
   n is 1 .. 2^25; more, or an unknown name, is refused with -1 and hx_last_error before anything is launched.  Returns 0.
   Synchronises. */
int hx_batch_debug_math(hx_batch *b, const char *name, const void *in, long long n, void *out);
/* Which route the calls of an hx_enc took since its last init (a successful or a rejected one; both reset the counters):
   out[0] = calls made the plain way, out[1] = calls replayed from the recorded graph, out[2] = the graph's state (0 = not
   recorded yet, 1 = ready, -1 = not available: HMP3AMD_ENC_GRAPH=0, or the recording failed and the calls go the plain way).
   Returns 0 (-1: null argument).  Changes nothing.  The contract tests/test_gpu_enc.py holds the encoder to:
   - the first two calls after an init are plain; from the third on hx_enc_L3_audio_encode and hx_enc_MP3_audio_encode are
     replays, whatever the control (every kernel family, a call that emits no byte, two frames or three), with the bytes and
     counters of the plain route;
   - the *_Packet calls, and every call under HMP3AMD_ENC_GRAPH=0 (read when an encoder first considers recording), are plain;
   - several live encoders - beside each other and beside a batch with a pipelined submit in flight - may be driven in any
     interleaving from one thread, and each from a thread of its own; one encoder is driven by one thread at a time. */
int hx_enc_debug_calls(hx_enc *e, int out[3]);
/* The first-generation allocator (intensity stereo, dual channel; reference bitallo1.cpp) calls libm's logf / log10f, which
   are not correctly rounded: what the reference encodes depends on the C library it is linked with.  The kernels restate
   glibc 2.35's (hmp3_amd/csrc/hx_libm32.h).  hx_libc_version: the host's C library; hx_libm_spot_check: how many of n
   sample arguments the host's logf / log10f treat differently (0: a reference built on this host and the kernels agree). */
const char *hx_libc_version(void);
int hx_libm_spot_check(int n);
/* The host build of the same restatement on arrays, for tests: "logf", "log10f", "a1_mask_db" and "a1_gz" of
   hx_batch_debug_math with the same patterns and operand layout ("a1_gz": the constants ec resolves to).  Returns 0;
   -1 for a rejected configuration, another name or a null argument.  Host only. */
int hx_debug_host_math(const HX_E_CONTROL *ec, const char *name, const void *in, long long n, void *out);
/* 1 if the host tables of this control have the structure the low-footprint kernel derives them from (gain tables and
   the x^(3/4) exponent table as ldexp of 4 / 16 constants, mB tables within 16 bits); hx_batch_create checks the same
   before it picks that kernel.  -1 = configuration rejected.  Host only. */
int hx_debug_slim_tables_ok(const HX_E_CONTROL *ec);
/* host-side table generation for the CPU tests (no GPU): see hx_host.cpp */
long long hx_debug_host_table(const HX_E_CONTROL *ec, const char *name, void *dst, long long cap);
/* For tests: the packing kernel on records of the caller's instead of the stream walk's, launched the way a batch's call
   launches it.  All pointers are host memory.  ec [ncls]: the controls of the classes in play; cls [S]: each stream's class;
   NG: granule positions per stream (even), fps: frame records per stream = NG with an MPEG-2 class among ec, else NG / 2;
   nfr [S] or null: per-stream frame counts (0 .. NG / 2).  seg [S][NG][2], ixq [S][NG][2][576], sgn [S][NG][2][20],
   frm [S][fps] and slots [S][fps + 40] in the layouts of hmp3_amd/csrc/hx_types.h (HxSegOut, quantised magnitudes, one sign
   bit per line, HxFrameOut - whose copies of the first four slots the call fills in itself - and HxSlot; the record sizes:
   hx_debug_host_table "sizeof_pack_records").  rows [S][out_stride] and packet [packet_bytes] (null: none) go to the device
   as the caller filled them and come back as the kernel left them; *status gets the kernel's status word.
   Every record is checked on the host first: one the stream walk cannot emit - a value above its table's range, segments
   that do not follow one another, more than 4095 bits in a segment, a slot outside its row or list ... - is refused with
   -1 and hx_last_error before anything is launched.  Returns 0. */
int hx_debug_pack(int device, const HX_E_CONTROL *ec, int ncls, const int *cls, int S, int NG, int fps, const int *nfr,
                  const void *seg, const short *ixq, const unsigned *sgn, const void *frm, const void *slots,
                  unsigned char *rows, long long out_stride, unsigned char *packet, long long packet_bytes, int *status);
/* For tests: the decoded-PCM kernels (k_recon_hybrid, k_recon_synth, k_recon_carry) on records of the caller's instead of
   the stream walk's, launched the way a batch's call launches them, with the tables a batch gives them.  All pointers are
   host memory.  ec [ncls]: the controls of the classes in play - MPEG-1 streams of the second-generation allocator only, any
   other class is refused by name as hx_batch_recon_buffer refuses it; cls [S]: each stream's class; NG: granule positions
   per stream (even); nfr [S] or null: per-stream frame counts (0 .. NG / 2).  ixq [S][NG][2][576], sgn [S][NG][2][20],
   seg [S][NG][2] and rec [S][NG / 2] in the layouts of hmp3_amd/csrc/hx_types.h (quantised magnitudes in bitstream order, one
   sign bit per line, HxSegOut - of which only sf is read, for short blocks: field 3 * band + window - and HxFrameDebug: ms,
   gr and sf; the record sizes: hx_debug_host_table "sizeof_recon_records").  state [S][1152 + 2 * 15 * 32] goes to the
   device as the caller filled it and comes back as k_recon_carry left it; hyb [S][NG][2][18 time slots][32 subbands], the
   hybrid output, and out [S][row], the rows in the layout of hx_batch_recon_buffer's, go the same way and come back as the
   kernels left them: what no kernel writes - blocks behind a stream's count, a mono stream's second channel - keeps the
   caller's bytes.
   Every record a kernel will read is checked on the host first: one the stream walk cannot hand over is refused with -1 and
   hx_last_error, which names stream, granule, channel and field, before anything is launched - block_type outside 0 .. 3,
   unequal in a granule's channels or not a legal successor of the granule before it; mixed_block_flag set; global_gain
   outside 0 .. 255; a subblock_gain outside 0 .. 7; a long scalefactor above 15 (bands 0 .. 10), 7 (11 .. 20) or 0 (21); a
   short field above 15 (bands 0 .. 5) or 7 (6 .. 11) or negative; a magnitude outside 0 .. 8206 within the coded range
   2 * big_values + 4 * aux_nquads (clipped at 576; nothing with aux_not_null 0); big_values above 288, aux_nquads negative;
   ms neither 0 nor 1; a count outside 0 .. NG / 2; a row shorter than a stream's blocks; state that is not finite.  What
   lies from the coded range on is not looked at: the kernels ignore it.  Returns 0.  Synchronises. */
int hx_debug_recon(int device, const HX_E_CONTROL *ec, int ncls, const int *cls, int S, int NG, const int *nfr,
                   const short *ixq, const unsigned *sgn, const void *seg, const void *rec, float *state, float *hyb,
                   float *out, long long row);
/* For tests: the stream walk's quantiser and Huffman counter - do_quant, quant_count_bits, count_bits, s_do_quant,
   s_count_bits_ch and what they call, unmodified - on records of the caller's.  One workgroup of two waves per record, as
   the walk has them: channel 1 runs on the helper wave, through the walk's work orders.  All pointers are host memory.
   unit names the build of the walk whose twin runs the records: "k_alloc", "k_alloc_slim", "k_alloc_lsf", "k_alloc1",
   "k_alloc1_lsf"; ec is a control whose streams that unit walks (its band tables are the records'), any other is refused.
   mode: 0 count            count_bits (the first-generation units: the channels one after the other, as their walk does)
         1 quant_count      quant_count_bits: quantise and count in one work order
         2 quant, count     do_quant, the clearing of channel 0's band-21 maximum if zero21, count_bits: the walk's route
                            while -HF lines are quantised in between
         3 short            s_do_quant, then s_count_bits_ch per channel
         4 short count      s_count_bits_ch per channel
   n records, 1 .. 16384.  hdr [n][16]: {block type 0 / 1 / 3, channels 1 / 2, ncb[2], opt, zero21, nsf[2], nbmax[2]}, the
   rest zero; the quantising modes alone read opt (0, 1, or 1 | 2; short: 0 or 1), zero21, nsf and nbmax (= the first line
   behind band nsf - 1); a short record has the channel count and opt only.  ix [n][2][576] (short: [n][2][3][192]): the
   lines as they stand before the call, and after it as the functions left them.  ixmax [n][2][22] (short: [n][2][3][16]):
   the band maxima, the same way.  x34 [n][2][576] and gsf [n][2][22] (short: [n][2][3][16]): magnitudes^(3/4) and gain
   steps, read by the quantising modes (null otherwise).  out [n][24]: per channel {table[4], cbreg[3], nbig, nquads, bits}
   as the counter left them (zeros for a channel that was not counted), then at [20] the returned sum.
   A record is checked on the host before anything is launched, its quantiser's result worked out there first, and refused
   with -1 and hx_last_error unless the walk could hand it over: lines and maxima 0 .. 8206, gain steps 0 .. 127, finite
   magnitudes that quantise to at most 8206, every line at most its band's maximum, lines at and past nbmax zero (band 21
   under opt & 2 excepted; the low-footprint unit without opt & 2 writes them itself and takes anything), count1
   quadruples of 0 and 1 only.  The last quadruple of channel 0 may reach lines 576 and 577 - channel 1's lines 0 and 1, as
   in the reference - in modes 0 and 2 of a two-channel record; in mode 1 the helper wave would be writing them.  Channel
   1's, or a mono record's, may not: the reference would read its sign bytes there, and no stream gets there on either
   channel - nothing is quantised above line 549 without -HF or above line 517 with it (check_count_long in
   hmp3_amd/csrc/hx_batch.hip has the argument) - so there is nothing to define.  Returns 0.  Synchronises. */
int hx_debug_count(int device, const HX_E_CONTROL *ec, const char *unit, int mode, int n, const int *hdr, int *ix, int *ixmax,
                   const float *x34, const int *gsf, int *out);
/* For tests: the stream walk's two certified band sums - the gain search (seek_actual: noise_sweep, the lanes' line runs, the
   segmented scan, the bucket certificate, the strict and the double-table fall-backs) and inverse_sf2, unmodified - on records
   of the caller's, by the kernels of hx_debug_count: one workgroup of two waves per record, channel 1 on the helper wave
   through the walk's work orders.  All pointers are host memory.  unit: "k_alloc", "k_alloc_slim" or "k_alloc_lsf" (the
   first-generation units run neither function and are refused); ec: a control whose streams that unit walks - its band
   tables and the line runs cut for its measured bands are the records'.  strict_sums 1: as a batch under
   HMP3AMD_EXACT_SUMS=1, no certificate passes.  n records, 1 .. 16384.
   hdr [n][16]: {nchan, nsf[2], nbmax[2], G[2], scale[2], 0 (short-block bands), 0 (-HF lines)}, the rest zero; a mono record
   has nsf[1] = nbmax[1] = 0.  xr [n][2][576]: the magnitudes.  band [n][2][22][8] and out [n][184]:
   mode 0 seek     x34 [n][2][576], x34max [n][2][22]; a band's words {NT, Noise0, gsf (the start step), gzero, NTadjust, 0, 0, 0};
                   out per (channel, band) {gsf, Noise, NTadjust, geval}
   mode 1 isf2     ix [n][2][576] the quantised lines; a band's words {up, lo, sf, ixmax, 0 ...}; G and scale in the header;
                   out per (channel, band) {sf, geval, 0, 0}
   and at out[176] the strict fall-backs the record's two waves counted (one per sweep with a band whose bucket was not
   proven; with strict_sums one per sweep), at out[177] the sweeps that took the double table.  Arrays of the other mode are
   null.  Every record is checked before anything is launched and refused with -1 and hx_last_error, which names record,
   channel, band and field, leaving out alone: nchan 1 or 2; nsf 1 .. the class's measured bands, nbmax the first line behind
   band nsf - 1 (both 0 for a channel the record does not have); the short-block and -HF words zero; lines and x34 finite,
   0 <= x34 <= 2^28; x34max the exact maximum of its band's x34, ixmax of its band's lines (0 .. 8206); start steps 0 .. 107
   (every step a search can evaluate then lies in the 128-entry gain tables: hmp3_amd/csrc/hx_types.h has the argument);
   gzero 0 .. 127; NT, Noise0, NTadjust within +-2^20; G 0 .. 255, scale 0 or 1, 0 <= lo <= up <= 255, sf 0 .. 255 (seek: G and
   scale zero).  Returns 0.  Synchronises. */
int hx_debug_seek(int device, const HX_E_CONTROL *ec, const char *unit, int mode, int strict_sums, int n, const int *hdr,
                  const float *xr, const float *x34, const int *ix, const int *band, const float *x34max, int *out);
/* For tests: K4 - k_spec (direct 0) or k_spec_direct (direct 1): hybrid MDCT, alias reduction, the long and short psy models
   and the L/R-vs-M/S metric before hysteresis, unmodified - on subband blocks of the caller's instead of k_polyphase's,
   launched the way a batch's call launches it (same grid, block size and slot arithmetic), with HxParams, HxGlobalTabs and
   HxStream staged as a batch stages them.  All pointers are host memory.  ec [ncls]: the controls of the classes in play, of
   any kind a batch accepts (MPEG-1 and MPEG-2 rates, both allocators, mono); cls [S]: each stream's class; NG: granule
   positions per stream (even), S * NG at most 65536; nfr [S] or null: per-stream frame counts (0 .. NG / 2).  sb [S][2][NG + 1][576]: the subband
   blocks in the kernel's layout (18 samples of subband 0, 18 of subband 1 ..., frequency inversion not applied); granule g
   reads blocks g and g + 1, so neighbouring granules share a block as they do in a call.  bt [S][NG]: the block types.
   xr [S][NG][2][576], etab [S][NG][128], thr [S][NG][128] and msbase [S][NG] go to the device as the caller filled them and
   come back as the kernel left them: what no wave writes - granules at or past 2 * nfr[s] - keeps the caller's bytes.
   Checked on the host before anything is launched, refused with -1 and hx_last_error, which names stream, granule, channel
   and field: a count outside 0 .. NG / 2; a block type outside 0 .. 3, or other than 0 in a stream of the first-generation
   allocator (intensity stereo, dual channel: it codes long blocks only), among a stream's 2 * nfr[s] granules; a sample that
   is not finite or above HX_SPEC_SAMPLE_MAX in magnitude among the 2 * nfr[s] + 1 blocks of either channel a wave reads.
   HX_SPEC_SAMPLE_MAX = 2^33: the reference's polyphase filter gives at most 2230539264 = 1.04 * 2^31 on the loudest input the
   parity tests feed (2^16 x full scale, tests/dynamic_range_cases.py; DESIGN.md has the measurement), rounded up to a power of
   two, 2^32, with one binade of margin.  No band sum of squares overflows at that bound: a line before the alias butterflies
   is a row of the windowed MDCT (18 x 36, absolute row sums at most 1.67 at every block type) times 36 samples, a butterfly
   adds at most |cs| + |ca| <= 1.38 times the larger of its two lines, so |line| < 2.3 * 2^33 < 2^35 and a square is below
   2^70; the widest band's 192 squares, the 100 in front, el + er and es + ed <= 4 (el + er) stay below 2^70 * 192 * 4 + 800
   < 2^80, far from FLT_MAX = 2^128, and so do the partition energies of the psy models (at most 576 squares).  Returns 0.
   Synchronises. */
#define HX_SPEC_SAMPLE_MAX 8589934592.0f
int hx_debug_spec(int device, const HX_E_CONTROL *ec, int ncls, const int *cls, int S, int NG, const int *nfr, int direct,
                  const float *sb, const unsigned char *bt, float *xr, float *etab, float *thr, int *msbase);

/* ---- Xing / Info / LAME tag frame (first frame of a file; reference pub/xhead.h) ----
   Same arguments and return values as the reference functions; the seek-table state that the
   reference keeps in file statics lives in an hx_xing object. */
typedef struct hx_xing hx_xing;
hx_xing *hx_xing_create(void);
void hx_xing_destroy(hx_xing *x);
/* xhead.c:255 XingHeader: builds the tag frame into buf, returns its size in bytes (0 = does not fit) */
int hx_xing_header(hx_xing *x, int samprate, int h_mode, int cr_bit, int original_bit, int flags, int frames,
                   int bs_bytes, int vbr_scale, const unsigned char *toc, unsigned char *buf,
                   const unsigned char *buf20, const unsigned char *buf20b, int kbps);
/* xhead.c:695 XingHeaderTOC: record a seek point; returns how many encode calls to wait for the next one */
int hx_xing_toc(hx_xing *x, int frames, int bs_bytes);
/* the seek points a ledger record holds (HX_LEDGER above) become x's, as if x had taken the record's hx_xing_toc calls */
int hx_xing_load_points(hx_xing *x, const HX_LEDGER *r);
/* xhead.c:486 XingHeaderUpdateInfo: final frame / byte counts, TOC, LAME info fields and CRCs; 1 = ok */
int hx_xing_update_info(hx_xing *x, unsigned frames, int bs_bytes, int vbr_scale, const unsigned char *toc,
                        unsigned char *buf, const unsigned char *buf20, const unsigned char *buf20b,
                        unsigned long long samples_audio, unsigned bytes_mp3, unsigned lowpass,
                        unsigned in_samplerate, unsigned out_samplerate, unsigned short musiccrc);
/* xhead.c:223 XingHeaderUpdateCRC (MusicCRC), xhead.c:236 XingHeaderBitrateIndex */
unsigned short hx_xing_update_crc(unsigned short crc, const unsigned char *data, int len);
/* host only: the CRC of A ++ B from crc_a = CRC(0, A), crc_b = CRC(0, B) and len_b = |B| >= 0, in O(log len_b):
   CRC(0, A ++ B) = crc_a * x^(8 len_b) mod P ^ crc_b (reflected CRC-16, polynomial 0xA001, bit 15 = x^0).  len_b = 0
   returns crc_a ^ crc_b (crc_b of an empty B is 0); a negative len_b is no length and returns crc_a unchanged. */
unsigned short hx_xing_crc_combine(unsigned short crc_a, unsigned short crc_b, long long len_b);
int hx_xing_bitrate_index(int mpeg1, int kbps);

#ifdef __cplusplus
}
#endif
#endif
