// hx_types.h - POD layouts shared by the host runtime and the HIP kernels of the
// MI355X batched MP3 encoder.  Domain names follow the reference (granule, sfb, part2_3...).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "hx_src.h"

// Same field order as the reference's E_CONTROL (pub/encapp.h:42-72): passed verbatim
// through the C-ABI.
struct HxControl {
    int mode, bitrate, samprate, nsbstereo, filter_select, freq_limit, nsb_limit;
    int layer, cr_bit, original, hf_flag, vbr_flag, vbr_mnr, vbr_br_limit, vbr_delta_mnr;
    int chan_add_f0, chan_add_f1, sparse_scale;
    int mnr_adjust[21];
    int cpu_select, quick, test1, test2, test3, short_block_threshold;
};

// MPEG_HEAD (pub/encapp.h:141-157)
struct HxMpegHead {
    int sync, id, option, prot, br_index, sr_index, pad, private_bit, mode, mode_ext, cr, original, emphasis;
};

// Psychoacoustic tables of one block class (long = 2 partitions per sfb)
struct HxPsyTab {
    int npart;          // spreading rows
    int npart_e;        // energy partitions
    int nsum[64];       // lines per partition
    int pstart[65];     // first line of partition
    int cnt[64], off[64], row[64];  // spreading row: length, first source partition, offset into w
    float w[2200];      // [0..63] absolute threshold x width, rows from 128
};

// Everything resolved at init for one configuration class (sample rate / bitrate / flags).
// Lives in device global memory; kernels index it through HxStream::cls.
struct HxParams {
    HxControl ec;           // echoed control (L3_audio_encode_info_ec)
    HxMpegHead head_info;
    unsigned char head[4];
    int totbitrate, samprate, sr_index, h_mode;
    int h_id, tix;          // 1 = MPEG-1, 0 = MPEG-2 LSF (one granule per frame); band-table row
    int nband, nsb, nsb_limit, nsb_ms0, nsb_ms1, band_limit, band_limit_stereo;
    int framebytes, remainder, divisor, main_framebytes, side_bytes, sf_bit_max, AveTargetBits;
    int ms_flag, hf_flag, vbr_flag, short_block_threshold, filter_dc;
    int nchan;              // 1 = mono (mode 3), 2 = stereo / joint stereo
    float filter_alpha;
    int ivbr_min, ivbr_max, vbr_main_framebytes[16], vbr_framebytes[16], vbr_pool_target;
    int initialMNR, test1, taperNT[22];
    int nBand_l_iso[22];
    int nBand_l[22], startBand_l[24], nBand_s[13], startBand_s[14];
    int nsf[2], nsf2[2], nsf3[2], nbmax[2], nbmax2[2], nbmax3[2];
    int look_log_cbwmb[22];
    float rnBand_l[22];
    unsigned char band_of_line[576];    // sfb index of each MDCT line (allocator's band table)
    // Blocked line runs of the stream walk's certified band sums (hx_alloc.hip, noise_sweep / inverse_sf2; hx_host.cpp band_runs):
    // lane l owns up to run_w consecutive lines of ONE band among the bands the gain search measures, the lanes of a band are
    // neighbours (at most 16).  lane_run[l] = first line >> 1 | (lines >> 1) << 9 | (lanes between l and its band's first lane) << 12;
    // band_last_lane[b] = the last lane of band b's run of lanes.
    int run_w;
    unsigned short lane_run[64];
    unsigned char band_last_lane[24];
    // 32-point analysis DCT: twiddles 2 cos(pi (2j+1) / 2N) of the size-N step at [N/2 + j] (heap order; [0] unused)
    float dct_tw[32];
    float win[4][36], csa[2][8];
    // N-point MDCT kernels (N = 18 long, 6 short): input twiddles, twiddles of the odd half, and the rows of the
    // N/2-point cosine transform that are not plain sums (9-point: outputs 2, 4, 8 / 1, 5, 7 / the factor of output 3)
    float mdct_pre18[18], mdct_odd18[9], dct9_even[3][4], dct9_odd[3][4], dct9_k3;
    float mdct_pre6[6], mdct_odd6[3], dct3_k;
    HxPsyTab psyL;
    HxPsyTab psyS;                      // short blocks: rows from w[0]
    float look_gain[128], look_34igain[128], look_ix43[256];
    // short-block allocator (reference bitallos.cpp:128-200)
    int nsfs, nbmax_s, look_log_cbwmb_s[16];
    unsigned char sband_of_line[192];   // short sfb index of each line of a 192-line window
    // streams the reference codes with its first-generation allocator (CBitAllo1, bitallo1.cpp): joint stereo with an
    // intensity part (is_flag) and dual channel.  Long blocks only; tables of bitallo1.cpp:107-211,444-543
    int is_flag, alloc1, a1_ill_is_pos;
    float a1_log_cbw[21];                       // 10 log10(band width)
    float a1_f_ix[256], a1_f_ixmax[256], a1_f_big_ix[256], a1_f_big_ixmax[256];    // noise estimators by quantised value
    int a1_bits[256], a1_is_pos[34];            // bit estimator x 16; intensity position by energy ratio
    float a1_gz0, a1_gz1, a1_gz2, a1_c707, a1_sparse[21];
};

// Class-independent tables.
#define HX_POW43_N 16384             // quantised values covered by the double-precision x^(4/3) table
struct HxGlobalTabs {
    double pow43[HX_POW43_N];           // i^(4/3) as the reference's pow() call returns it (noise of lines quantised beyond the 256-entry float table)
    float anwin[512];
    float anwin_r[512];                 // the same window in the order K1 uses it: [k][j][A tap, B tap]
    int mblog[256];
    float mbexp_lo[256], mbexp_hi[256];
    float pow34_exp[256], pow34_a[16], pow34_b[16];
    float quant_off[32];
    int logsub[84];
    unsigned short huff_code[1408];     // 1378 used (ISO Table B.7 at true dimensions)
    unsigned char huff_len[1408];
    unsigned short huff_off[32];
    unsigned char huff_dim[32], huff_lin[32];
    unsigned char quada_code[16], quada_len[16];
};

// Tables of the decoded-PCM kernels (hx_recon.hip; hx_host.cpp hx_recon_tabs builds them in double from their closed forms
// and from anwin): what an ISO 11172-3 decoder's back half multiplies by.
struct HxReconTabs {
    double pow2q[4];            // 2^(k / 4): the fractional part of a requantisation exponent
    float cos36[36][18];        // cos(pi / 72 (2 i + 19) (2 k + 1)): the 36-point IMDCT, output i, line k
    float cos12[12][6];         // cos(pi / 24 (2 i + 7) (2 k + 1)): the 12-point IMDCT
    float win[4][36];           // the windows of block types 0 .. 3 (type 2: 12 taps)
    float cs[8], ca[8];         // alias reduction butterflies
    float synth[32][64];        // [k][i] cos((16 + i) (2 k + 1) pi / 64): the synthesis bank's matrixing, transposed
    float dwin[512];            // the synthesis window D[n] = 32 C[n], times 32768 (the output is at int16 scale)
};
// Carried state of a stream's decoded PCM, floats: the previous granule's IMDCT tails [2][32][18], then the last 15 time
// slots of hybrid output [2][15][32], oldest first (hx_batch::d_recon_state, [S] of these)
#define HX_RECON_TAIL_FLOATS (2 * 576)
#define HX_RECON_HIST_SLOTS 15
#define HX_RECON_STATE_FLOATS (HX_RECON_TAIL_FLOATS + 2 * HX_RECON_HIST_SLOTS * 32)

// Side information of one granule/channel (pub/l3e.h:72-96)
struct HxGr {
    int part2_3_length, big_values, global_gain, scalefac_compress;
    int window_switching_flag, block_type, mixed_block_flag;
    int table_select[3], subblock_gain[3];
    int region0_count, region1_count, preflag, scalefac_scale, count1table_select;
    int aux_nquads, aux_bits, aux_not_null, aux_nreg[3];
};

#define HX_MAINBUF (16384 + 512 + 1440 + 256)

// Persistent per-stream state (device global memory).  It is the checkpoint unit: copying
// this struct plus the subband carry is a complete snapshot of a stream.
struct HxStream {
    int cls;                    // index into the HxParams array
    int frames_in;              // frames submitted so far
    // front end
    float dc[2];
    float pcm_hist[2][480];     // last 480 filtered samples per channel (oldest first)
    int attack_hist[2][32];     // energy history in mB (detect.c)
    int bt_prev;                // block type of the previous granule
    int short_flag_next_prev;   // short_flag_next of the previous granule
    float thr_prev[2][64];      // previous granule's unclamped thresholds x 2 (ecsave)
    // allocator
    int MNR, PoolFraction, call_count, ms_memory, NTadjust[2][22];
    // first-generation allocator (pub/bitallo1.h:80-140): gain steps carried per channel, bit-estimate feedback,
    // running noise-to-mask level
    int a1_gsf[2][21], a1_bitadjust[2], a1_call_count;
    float a1_running_a, a1_ave_alpha, a1_alpha;
    int sf_save[2][21];
    int gr_subblock_gain[2][2][3];
    // reservoir / frame assembly (mp3enc.cpp:2230-2333)
    int padcount;
    unsigned main_tot, main_sent, mf_tot;
    int main_bytes, main_p0, main_p1;
    unsigned side_p0, side_p1;
    unsigned frame_main_pos[32];
    int frame_mf_bytes[32];
    unsigned char mode_ext_buf[32], br_index_buf[32], side_buf[32][32];
    unsigned tot_frames_out, tot_bytes_out;
    int ave_tot_bytes_out;
    unsigned char main_buf[HX_MAINBUF];
};

// What the allocator needs at the start of a long-block granule and that does not depend on its carried state:
// written by k_prep per (stream, granule), read by k_alloc.  Energies are those of the input channels (L / R);
// x34max / gzero refer to the representation the frame is coded in (L / R, or M / S in a joint-stereo frame).
struct alignas(16) HxBandPrep {
    float xsxx[2][22];          // band energies of L and R
    float x34max[2][22];        // largest |x|^(3/4) of the band
    int n0[2][22];              // band energy per line in mB: L, R
    int n0ms[2][22];            // the same of M, S (joint-stereo frames only)
    int gzero[2][22];           // gain step at which the whole band quantises to zero
    int maskmb[2][22];          // masking threshold in mB after pre-echo control
};

// Optional per-frame debug taps written by the allocator kernel (tests only).
struct HxFrameDebug {
    int ms, ms_metric[2], byte_pool, MNR_after;
    int mask_mb[2][2][22];      // unused: no kernel writes it (kept for the layout, which two test mirrors share); the masks after pre-echo control are HxBandPrep.maskmb, the "band" tap
    HxGr gr[2][2];
    int sf[2][2][22];
    int scfsi[2];
    int main_bytes;             // bytes of main data produced by this frame (before padding)
};

// ---- k_alloc -> k_pack hand-over: what the packer needs of a coded frame ----
// One (granule, channel): where its bits start in the frame's main data, the scalefactor fields in transmission
// order, the Huffman regions.  The quantised lines travel as int16 beside it.
struct alignas(16) HxSegOut {
    int start_bit;              // first bit of the segment within the frame's main data
    int huff_bits;              // Huffman bits counted by the allocator (the packer checks them)
    unsigned nreg01;            // pairs in region 0 | pairs in region 1 << 16
    unsigned nreg2_quads;       // pairs in region 2 | count1 quads << 16
    unsigned tabs;              // Huffman table of region 0 | region 1 << 8 | region 2 << 16 | count1 table << 24
    int not_null;               // 0 = the segment carries no bits at all
    unsigned short sf[40];      // (length << 8) | value of each transmitted scalefactor field
};
// One frame: its main data spans the pending slots from first_slot on (the first one has main_bytes bytes in use)
struct HxSlot { int off, mf; };     // a frame's slot in a stream's output: offset of its header, main-data bytes it holds
struct alignas(16) HxFrameOut {
    int bytes, raw_bytes;       // main data bytes with / without the zero stuffing up to byte_min
    int first_slot, main_bytes;
    long long packet_off;       // offset of the frame's main data in the packet buffer, -1 = no packet
    int pad_[2];
    HxSlot near[4];             // copies of slots first_slot .. first_slot + 3: the packer rarely needs more, and gets them in the record's round trip
};
#define HX_SLOTS_EXTRA 40           // slots pending from earlier calls (the ring holds 32)

// k_polyphase (hx_polyphase.hip) and its launch (hx_batch.hip): granules per workgroup (252 of 256 lanes busy: a lane is a time slot
// of a granule) and the workgroup size that follows.  One definition: the kernel's launch bounds, its LDS staging stride and
// register array are sized by the same numbers the host launches with.
// (7 granules: 126 of the workgroup's 128 lanes have a time slot, 37 KB of LDS, four workgroups per CU; with 14 - 252 of 256 lanes,
// 70 KB, two per CU - the loads of one workgroup's tile overlapped less of the other's arithmetic: 7 is +1.6 % per step at configs 2
// and 3; 3 and 5 granules are level with it, 10 in between)
#ifndef K1_GPB
#define K1_GPB 7
#endif
#define K1_THREADS ((K1_GPB * 18 + 63) / 64 * 64)

// The lines' signs travel from k_prep (or, for short-block and first-generation-allocator granules, the stream walk) to
// k_pack as one bit per line: 576 bits = 18 words per (granule, channel), padded to 20 so that a granule's 160 bytes keep
// 16-byte alignment.  (As one byte per line they were 0.6 GB written and 0.6 GB read per config-2 step.)
#define HX_SGN_WORDS 20

// The dense image (hx_batch_dense_buffers): a workgroup of k_dense_gather (hx_pack.hip) moves this many bytes of one row -
// 256 lanes x 4 vectors of 16 bytes; the host sizes the grid with it from the worst-case row.
#define HX_DENSE_CHUNK 16384
// PCM segments (hx_batch_pcm_segments): a workgroup of k_pcm_spread (hx_pcmin.hip) moves this many bytes of one segment, the
// same way; the host sizes the grid with it from the call's row.
#define HX_PCM_CHUNK 16384
// File images (hx_batch_file_images): a workgroup of k_file_append (hx_fileimg.hip) moves this many bytes of one image, the
// same way; the host sizes the grid with it from the worst-case row plus the 15 bytes a piece may start off a vector.
#define HX_FILE_CHUNK 16384
// The fetch of many files (hx_batch_file_fetch_many): a workgroup of k_file_gather (hx_fileimg.hip) moves this many bytes of
// one listed image, the same way; the host sizes the grid with it from the images' pitch.
#define HX_FILE_GATHER_CHUNK 16384

// Slots of a batch's counter block (AllocArgs::done_counter; the host runtime reads some of them and hands two to k_gate and k_pack).
enum HxCounter {
    HX_CNT_RETIRED = 0,         // streams retired
    HX_CNT_GATE_TIMEOUTS = 1,   // gates (k_gate) that gave up waiting
    HX_CNT_STARTED = 2,         // streams started by all allocator launches of the batch (wraps): the gates wait on it, the one-stream
                                // encoder's packing publishes it as the call's sequence word
    HX_CNT_BIG_SWEEPS = 3,      // gain-search line passes that took the double x^(4/3) table
    HX_CNT_STRICT_SUMS = 4,     // certified band sums that fell back to the strict line-order sum
    HX_CNT_CLAIMED = 5,         // positions of the launch order claimed so far in this launch (persistent workgroups)
    HX_CNT_IDLE = 6,            // workgroups of this launch that ran out of work (the last one zeroes this and the claim counter)
    HX_CNT_PARK = 8,            // [HX_CNT_PARK ..]: the CU ids of the parking scheme, one per parked position (hx_alloc3.inc)
    HX_CNT_LUCKY = 72,          // [3] big_lucky_noise of the 256-register stream walks: granules it measured, its passes, granules
                                // one of whose passes held more than six candidates per band
    HX_CNT_LUCKY_ROUNDS = 75,   // [3] big_lucky_noise's work lists (every stream walk): entries summed, rounds of 64 entries beyond a
                                // wave's first, the longest list of a pass
};
#define HX_PARK_MAX 64
#define HX_CNT_WORDS (HX_CNT_LUCKY_ROUNDS + 3)
static_assert(HX_CNT_LUCKY == HX_CNT_PARK + HX_PARK_MAX, "the big_lucky counters follow the parking scheme's words");

// What k_debug_math (hx_alloc1.inc; tests only, hx_batch_debug_math) evaluates: the device functions of the kernels on
// arguments of the caller's, one per lane.  The name table and each function's operand count are in hx_batch.hip.
enum HxDebugMath {
    HX_DM_LOGF, HX_DM_LOG10F, HX_DM_A1_MASK_DB, HX_DM_A1_GZ, HX_DM_DBLOG, HX_DM_DUAL_G, HX_DM_IS_SCALE, HX_DM_IS_SCALE_LSF,
    HX_DM_DIV, HX_DM_MBLOG, HX_DM_MBLOG16, HX_DM_MBEXP, HX_DM_POW34, HX_DM_ROUND, HX_DM_COUNT
};
#define HX_DEBUG_MATH_MAX (1LL << 25)   // arguments per call

// Slots of the stream walk's profile (built with -DHX_PROFILE: AllocArgs::prof, 64 per stream; tools/prof_slots.py reads this
// table for the profile tools).  Master-wave clock64 ticks booked to a phase, except the counts (HX_PROF_N_*).
enum HxProf {
    HX_PROF_JOIN_FETCH = 0,         // frame loop: wait for the helper's fetch of the granule's operands, band start values out of the landing area
    HX_PROF_STARTUP = 1,            // long granule: startup_prepped
    HX_PROF_SEEK_INITIAL = 2,
    HX_PROF_SEEK_ACTUAL = 3,
    HX_PROF_TRADE_DUAL = 4,
    HX_PROF_SCALE_FACTORS = 5,
    HX_PROF_BIG_LUCKY = 6,
    HX_PROF_DO_QUANT = 7,
    HX_PROF_QUANT_COUNT = 8,        // quantise-and-count, or the count after do_quant
    HX_PROF_INCREASE_BITS = 9,
    HX_PROF_DECREASE_BITS = 10,
    HX_PROF_INVERSE_SF2 = 11,
    HX_PROF_BITALLO = 12,           // frame loop: the granule's allocation
    HX_PROF_HANDOVER = 13,          // frame loop: the granule's segments sized and handed to the outbox
    HX_PROF_BUDGET = 14,            // frame loop: the frame's budget
    HX_PROF_GR_PRE = 15,            // frame loop: short-block mask, block types
    HX_PROF_FETCH_POST = 16,        // frame loop: the next granule's fetch order
    HX_PROF_EMIT = 17,              // frame placement: packets, debug taps
    HX_PROF_RETIRE = 18,            // frame placement: full slots retired, running totals
    HX_PROF_PACK_SF = 19,           // hand-over: scalefactor sizing of one channel
    HX_PROF_N_SWEEPS = 20,          // count: gain-search sweeps of the master wave
    HX_PROF_N_LUCKY = 21,           // count: big_lucky passes
    HX_PROF_N_COUNTS = 22,          // count: bit counts
    HX_PROF_LUCKY_SETUP = 23,
    HX_PROF_LUCKY_EVAL = 24,        // the entries' noise terms, formed and added
    HX_PROF_LUCKY_REPLAY = 26,
    HX_PROF_SWEEP_PUBLISH = 27,     // gain-search sweep: band lanes publish their gain pairs
    HX_PROF_SWEEP_LINES = 28,
    HX_PROF_SWEEP_SUMS = 29,
    HX_PROF_SEEK_JOIN = 30,         // gain search: wait for the helper's channel
    HX_PROF_TOTAL = 31,             // the stream's whole walk
    HX_PROF_CNT_BALLOTS = 36,       // count_bits_ch: ...
    HX_PROF_CNT_J23 = 37,
    HX_PROF_CNT_REGIONS = 38,
    HX_PROF_CNT_PAIRS = 39,
    HX_PROF_CNT_QUADS = 40,
    HX_PROF_CNT_REDUCE = 41,
    HX_PROF_QC_POST = 42,           // quant_count_bits: the helper's order, the quantiser, the join
    HX_PROF_QC_QUANT = 43,
    HX_PROF_QC_JOIN = 44,
    HX_PROF_N_SWEEPS_HELPER = 45,   // count: gain-search sweeps of the helper wave (channel 1)
    HX_PROF_GR_TAIL = 46,           // frame loop: the granule loop's tail
    HX_PROF_PL_SIZES = 47,          // frame placement: size, bitrate index
    HX_PROF_PL_SLOT = 48,           // frame placement: slot and frame record
    HX_PROF_PL_HEAD = 49,           // frame placement: header, side information copy
};
#define HX_PROF_WORDS 64            // slots per stream

// Arguments of the allocator kernels (k_alloc / k_alloc_lsf), filled by the host runtime.
struct AllocArgs {
    HxStream *st;
    const HxParams *prm;
    const HxGlobalTabs *gt;
    const float *xr;            // [S][NG][2][576]
    const float *etab, *thr;    // [S][NG][2][64]
    const int *msbase;          // [S][NG]
    const unsigned char *bt;    // [S][NG]
    const unsigned char *btprev;    // [S] block type of the granule before this call
    unsigned char *out;         // [S][out_stride]
    int *out_bytes;             // [S]
    HxFrameDebug *dbg;          // [S][F] or null
    long long out_stride;
    int NG, S;                  // NG: granules of the call = the row stride of every [S][NG] array
    const int *nfr;             // [S] frames each stream takes of this call (hx_batch_frame_counts: stream s walks 2 nfr[s] granules
                                // of its row), or null = NG / 2 each
    int *status;
    unsigned long long *prof;
    unsigned char *packet;      // optional [S][F][packet_stride]: each frame as a self-contained packet
    long long packet_stride;
    int *packet_bytes;          // [S][F]
    int *frame_stats;           // optional [S][F][2]: frames / bytes emitted by the stream after each input frame
    int *pre_len, *carry_len;   // [S] bytes of pending frames' images at the call's start (k_pack_pre copies them in) / at its end (k_pack_carry saves them)
    const int *order;           // workgroup -> stream (longest-running first, from the previous call's durations), or null = identity
    unsigned *dur;              // [S] this call's duration of each stream's workgroup, 100 MHz ticks
    int *done_counter;          // [HX_CNT_WORDS] the batch's counter block (HxCounter)
    int park_k;                 // > 0: the workgroups that share a CU with one of the first park_k workgroups of the launch order (the streams that ran
                                // longest in the previous call) keep their slot until that one retires (hx_alloc3.inc, "parking")
    int strict_sums;            // 1 = no certified band sums: every band is added in line order (HMP3AMD_EXACT_SUMS=1; tests)
    // from k_msscan (hx_spec.hip) / k_prep (hx_prep.hip); xr holds the coded magnitudes for long-block granules
    const float *x34;           // [S][NG][2][576] x^(3/4) of the magnitudes (long-block granules)
    const unsigned *sgn;        // [S][NG][2][HX_SGN_WORDS] sign of each line, one bit per line in line order (bit j & 31 of word j >> 5)
    const HxBandPrep *band;     // [S][NG]
    const unsigned char *msflag;    // [S][NG] 1 = the granule's frame is coded M/S
    const int *msdec;           // [S][NG] the stereo metric after hysteresis (debug taps)
    const float *thrprev;       // [S][2][64] pre-echo memory the call started with
    // to k_pack (hx_pack.hip)
    short *ixq;                 // [S][NG][2][576] quantised magnitudes
    unsigned *sgn_w;            // the sign buffer again, writable: short-block granules store their reordered signs
    HxSegOut *seg;              // [S][NG][2]
    HxFrameOut *frm;            // [S][fpc]
    HxSlot *slots;              // [S][fpc + HX_SLOTS_EXTRA]
    // The launch's span of the batch-wide launch order: positions pos0 .. pos0 + npos - 1 (`order` [S] maps a position to its
    // stream; null = identity).  A batch of one kind walks 0 .. S - 1 in one launch; a batch of several kinds makes one launch
    // per kind, each over that kind's span of the order k_order_kinds made (hx_batch.hip, launch_walk).
    int pos0, npos;
    // fpc: frame records per stream = the stride of frm and (+ HX_SLOTS_EXTRA) of slots, one value for every walk kernel of a
    // call and for k_pack, which reads them: NG / 2 when every class of the batch is MPEG-1, else NG (an MPEG-1 stream of such
    // a batch uses the first NG / 2 of its row)
    int fpc;
};

// ---- k_debug_count_* (hx_alloc3.inc; tests only, hx_debug_count): the stream walk's quantiser and Huffman counter on
// records of the caller's, one workgroup per record.  What a record holds, per mode (hx_batch.hip checks every one before
// a launch; include/hmp3_amd.h describes them for the caller):
enum HxDebugCount {
    HX_DC_COUNT,            // count_bits on given lines and band maxima (first-generation units: a1_count_channels)
    HX_DC_QUANT_COUNT,      // quant_count_bits: one work order to the helper wave
    HX_DC_QUANT_THEN_COUNT, // do_quant, the M/S clearing of band 21's maximum, count_bits: the route under -HF
    HX_DC_SHORT,            // s_do_quant, then s_count_bits_ch per channel
    HX_DC_SHORT_COUNT,      // s_count_bits_ch per channel on given lines and maxima
    HX_DC_MODES
};
// header words of a record
enum { HX_DCH_BT, HX_DCH_NCHAN, HX_DCH_NCB0, HX_DCH_NCB1, HX_DCH_OPT, HX_DCH_ZERO21, HX_DCH_NSF0, HX_DCH_NSF1, HX_DCH_NBMAX0, HX_DCH_NBMAX1, HX_DCH_WORDS = 16 };
// result words of a record: per channel the counter's ten outputs, then the returned sum
enum { HX_DCO_TABLE = 0, HX_DCO_CBREG = 4, HX_DCO_NBIG = 7, HX_DCO_NQUADS = 8, HX_DCO_BITS = 9, HX_DCO_CH = 10, HX_DCO_SUM = 20, HX_DCO_WORDS = 24 };
#define HX_DEBUG_COUNT_MAX 16384    // records per call
struct HxCountArgs {
    int mode, n;
    int nband;              // band maxima / gain steps per channel: 22 of a long record, 48 = [3][16] of a short one
    const int *hdr;         // [n][HX_DCH_WORDS]
    int *ix;                // [n][2][576] lines: as they stand before the call, as the functions left them after it
    int *ixmax;             // [n][2][nband] band maxima, the same way
    const float *x34;       // [n][2][576] (the quantising modes)
    const int *gsf;         // [n][2][nband] gain steps (the quantising modes)
    int *out;               // [n][HX_DCO_WORDS]; the noise modes: [n][HX_DSO_WORDS]
    // the noise modes (below) only
    const float *xr;        // [n][2][576] magnitudes
    const int *band;        // [n][2][22][HX_DSB_WORDS]
    const float *x34max;    // [n][2][22] (seek)
};

// ---- the same kernels' noise modes (hx_debug_seek): the walk's two certified band sums - the gain search seek_actual and
// inverse_sf2, with everything they call - on records of the caller's.  HxCountArgs::mode goes on where HxDebugCount ends; hdr,
// x34 (seek), ix (isf2: read only) and out are HxCountArgs' own, in the layouts below.  The first-generation units have neither
// function.  include/hmp3_amd.h describes a record for the caller, hx_batch.hip (check_seek_record) has the rule of every field.
enum HxDebugSeek { HX_DS_SEEK = HX_DC_MODES, HX_DS_ISF2, HX_DS_END };
// header words of a record; NSFS and HF stand for the short-block and -HF fields of the walk, which neither function reads: zero
enum { HX_DSH_NCHAN, HX_DSH_NSF0, HX_DSH_NSF1, HX_DSH_NBMAX0, HX_DSH_NBMAX1, HX_DSH_G0, HX_DSH_G1, HX_DSH_SCALE0, HX_DSH_SCALE1,
       HX_DSH_NSFS, HX_DSH_HF, HX_DSH_WORDS = 16 };
// words of a band (seek | isf2)
enum { HX_DSB_NT = 0, HX_DSB_NOISE0, HX_DSB_GSF, HX_DSB_GZERO, HX_DSB_NTADJUST, HX_DSB_WORDS = 8 };
enum { HX_DSB_UP = 0, HX_DSB_LO, HX_DSB_SF, HX_DSB_IXMAX };
// A gain step of a seek record, bands below nsf: every step the search can evaluate from start step s must index the 128-entry
// gain tables, and the kernel clamps its indices for the reads that run a sweep ahead only.  Walking down it measures
// s - 1 .. s - min(s - 1, 20), which is >= 1 whatever s >= 0 is; walking up it measures s + 1 .. s + 20.  So 0 <= s <= 107 is
// the whole rule, and it needs no search to state.
#define HX_DS_GSF_MAX 107
// x^(3/4) of a seek record's line: at most 2^28, so that its quantised value at the largest 1 / gain^(3/4) (2^1.5, step 0) is
// an int - the conversion of a larger float is undefined in C, which the oracle and the reference are written in
#define HX_DS_X34_MAX 268435456.0f
#define HX_DS_INT_MAX (1 << 20)     // targets, start noise, estimator feedback: |v| at most this (no sum of them overflows)
// result words of a record: per (channel, band) four - seek {gsf, Noise, NTadjust, geval}, isf2 {sf, geval, 0, 0} - then the
// stream's count of strict fall-backs (AllocLds::nstrict) and the double-table passes (what the walk adds to HX_CNT_BIG_SWEEPS)
enum { HX_DSO_BAND = 4, HX_DSO_NSTRICT = 2 * 22 * 4, HX_DSO_BIG, HX_DSO_WORDS = 2 * 22 * 4 + 8 };


// ---- slot operations (hx_slots.hip: k_slot_reset / k_slot_gather / k_slot_scatter) ----
// One listed slot of an operation: the slot, the receiving batch's class of it, the configuration fingerprint a
// stream-state blob of it carries (gather) or must carry (scatter) and, of a converting batch, its converter plan.  cls and
// plan are what the slot runs once the operation is done: a reset stamps them into the slot (hx_batch_assign_streams hands
// it another menu entry's, hx_batch_reset_streams the present one's).
struct HxSlotEntry { int slot, cls; unsigned long long cfg; int plan, pad; };
// A stream-state blob, the one description of its layout.  A header {magic of the batch's kind, format version,
// sizeof(HxStream), 0, fingerprint of the stream's resolved configuration}: a blob from another library build (other state
// layout) or saved under another control is refused instead of silently yielding a corrupt bitstream.  Then the parts, each
// at its byte offset: HxStream, the three carried subband granules of channels 0 and 1, and (a converting batch's blob: another
// magic, neither kind takes the other's) the converter's plan fingerprint, call count and carried case-4 samples.
struct HxStateHeader { unsigned magic, version, state_bytes, pad; unsigned long long cfg; };
#define HX_STATE_MAGIC 0x53335848u          // "HX3S"
#define HX_STATE_MAGIC_SRC 0x43335848u      // "HX3C"
#define HX_STATE_VERSION 3u
#define HX_STATE_CARRY_BYTES (3 * 576 * sizeof(float))       // per channel
#define HX_STATE_SRC_CARRY_BYTES (2 * HX_SRC_CARRY * sizeof(float))
#define HX_STATE_OFF_STREAM sizeof(HxStateHeader)
#define HX_STATE_OFF_CARRY (HX_STATE_OFF_STREAM + sizeof(HxStream))
#define HX_STATE_END (HX_STATE_OFF_CARRY + 2 * HX_STATE_CARRY_BYTES)      // the end of a plain batch's blob
#define HX_STATE_OFF_SRC_FP HX_STATE_END
#define HX_STATE_OFF_SRC_CALLS (HX_STATE_OFF_SRC_FP + sizeof(unsigned long long))
#define HX_STATE_OFF_SRC_CARRY (HX_STATE_OFF_SRC_CALLS + sizeof(long long))
#define HX_STATE_END_SRC (HX_STATE_OFF_SRC_CARRY + HX_STATE_SRC_CARRY_BYTES)      // the end of a converting batch's
// ... and in 8-byte words, the unit the kernels move.  The header's words by the fields they hold: {magic, version},
// {state_bytes, pad}, cfg; the parts behind it are counted from the start of HxStream.
#define HX_SLOT_HDR_WORDS 3
#define HX_SLOT_HDR_MAGIC ((int) (offsetof(HxStateHeader, magic) / 8))
#define HX_SLOT_HDR_STATE_BYTES ((int) (offsetof(HxStateHeader, state_bytes) / 8))
#define HX_SLOT_HDR_CFG ((int) (offsetof(HxStateHeader, cfg) / 8))
#define HX_SLOT_ST_WORDS ((int) (sizeof(HxStream) / 8))
#define HX_SLOT_CARRY_WORDS ((int) (HX_STATE_CARRY_BYTES / 8))      // per channel
#define HX_SLOT_SRC_WORD ((int) ((HX_STATE_OFF_SRC_FP - HX_STATE_OFF_STREAM) / 8))     // plan fingerprint; the call count is the next word
#define HX_SLOT_SRC_CARRY_WORD ((int) ((HX_STATE_OFF_SRC_CARRY - HX_STATE_OFF_STREAM) / 8))
#define HX_SLOT_SRC_CARRY_WORDS ((int) (HX_STATE_SRC_CARRY_BYTES / 8))
static_assert(sizeof(HxStateHeader) == 8 * HX_SLOT_HDR_WORDS && offsetof(HxStateHeader, version) == 8 * HX_SLOT_HDR_MAGIC + 4 &&
              offsetof(HxStateHeader, pad) == 8 * HX_SLOT_HDR_STATE_BYTES + 4, "the header is three 8-byte words: {magic, version}, {state_bytes, pad}, cfg");
static_assert(HX_STATE_OFF_STREAM % 8 == 0 && HX_STATE_OFF_CARRY % 8 == 0 && HX_STATE_CARRY_BYTES % 8 == 0 && HX_STATE_OFF_SRC_FP % 8 == 0 &&
              HX_STATE_OFF_SRC_CALLS % 8 == 0 && HX_STATE_OFF_SRC_CARRY % 8 == 0 && HX_STATE_END_SRC % 8 == 0, "every part of a blob starts on an 8-byte boundary");
// ---- the file ledger (hx_ledger.hip: k_ledger / k_ledger_begin / k_ledger_gather; the record: HX_LEDGER, include/hmp3_amd.h) ----
// One listed slot of hx_batch_ledger_begin (the file's parameters) or of a read (the slot alone).  It travels through the
// slot operations' staging, whose copies hold [S] HxSlotEntry.
// fpc: the frames per call (1152-sample block) of the entry the slot runs when the record begins: 1, or 2 at the MPEG-2 rates.
struct HxLedgerEntry { int slot, ncalls, head_bytes, flags, fpc; };
static_assert(sizeof(HxLedgerEntry) <= sizeof(HxSlotEntry), "a ledger list fits the slot operations' staging");
// One listed slot of hx_batch_file_tags: the slot and its tag's description (HX_FILE_TAG, include/hmp3_amd.h, as six 8-byte
// words: this header stays free of the public one).  The list travels through a staging of its own, [S] entries per copy, in
// the slot operations' rotation.
struct HxFileTagEntry { int slot, pad[3]; unsigned long long tag[6]; };
static_assert(sizeof(HxFileTagEntry) == 64, "a tag entry is four 16-byte vectors");
#define HX_FILE_TAG_MAX 1440                        // the largest tag frame: 320 kbit/s at 32 kHz
#define HX_LEDGER_KEPT 512                         // seek points before a decimation halves them (hx_xing_toc)
#define HX_LEDGER_HDR_WORDS 16                      // 4-byte words in front of the points

#define HX_SLOT_VEC 4                               // words per lane
#define HX_SLOT_CHUNK (256 * HX_SLOT_VEC)           // words per workgroup
struct SlotArgs {
    const HxSlotEntry *ent;     // [n], entry e = blockIdx.x / chunks
    HxStream *st;               // [S]
    const HxStream *init;       // [classes] the state a new stream of the class starts with (k_slot_reset)
    float *sb;                  // the subband buffer; sb_row floats per (stream, channel), the carry in the first 3 * 576
    long long sb_row;
    long long *src_calls;       // converting batches: [2][S] call counts, [2][S][2][HX_SRC_CARRY] carried samples and [S] plan
    float *src_carry;           // fingerprints; src_par = the copy the next call reads.  src_calls null: no converter part
    unsigned long long *src_fp;
    int *src_cls;               // [S] stream -> plan, as k_src reads it, and [plans] each plan's fingerprint: k_slot_reset
    const unsigned long long *plan_fp;      // writes the slot's word of src_cls and of src_fp from its entry's plan
    int S, src_par;
    unsigned magic, version;    // of the batch's kind of blob
    int *status;                // bit 32: k_slot_scatter refused a blob
    int chunks;                 // workgroups per entry
    long long blob_words;       // blob_stride / 8
    float *recon_state;         // [S][HX_RECON_STATE_FLOATS] the decoded PCM's carried state, which k_slot_reset zeroes for the
                                // listed slots, or null: the batch never had hx_batch_recon_buffer switched on
};
