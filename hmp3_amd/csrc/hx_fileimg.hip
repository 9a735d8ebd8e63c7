// hx_fileimg.hip - file images (include/hmp3_amd.h, "file images"): k_file_append puts the bytes of a call that the ledger gave
// to a file behind the file's bytes so far, in the slot's image; k_file_begin restarts a slot's length word; k_ledger_brief
// writes the short form of every record; k_file_tag builds a file's tag frame into its image's head room; k_file_off and
// k_file_gather bring any number of images together as one dense image (all three: the end of this file).  Built as part of
// hx_pack.hip's unit, behind hx_pcmin.hip (and behind hx_crc.hip and hx_ledger.hip, whose CRC arithmetic k_file_tag uses).
//
// Slot s's image is `pitch` bytes at img + s * pitch (img from hipMalloc, pitch a multiple of 16: every image starts on a
// 16-byte boundary), of which the first cap count.  Beside the ledger the slot has one pair of words, fw[s]: x = image_bytes,
// the audio bytes present in the image; y = 1 when the slot's record was begun while images were on.
//
// k_file_append runs right behind k_ledger and reads the record as k_ledger has just left it.  Workgroup (stream s, chunk c):
//   - leaves at once unless the stream takes n > 0 frames of the call, fw[s].y is set, the record is open and its call_bytes
//     is positive.  (k_ledger writes call_bytes for every open record of a stream with n > 0 - 0 for one that had ended - so
//     with n > 0 the word is this call's; with n = 0 it is the previous call's and is not looked at.  The host does not launch
//     the kernel for a call without counters and CRCs, whose live records k_ledger leaves alone; the one other record k_ledger
//     leaves alone, a live one with a seek-point state out of range, is left alone here by the same test.)
//   - the piece: L = call_bytes bytes from the start of row s go to image bytes [at, at + L), at = head_bytes + bytes - L;
//     what lies at or beyond cap is cut off: Lc = min(L, cap - at), and a workgroup with Lc <= 0 leaves;
//   - works in destination-aligned 16-byte vectors: with dm = at & 15, vector j is image bytes [at - dm + 16 j, + 16) and
//     holds row bytes [16 j - dm, 16 j - dm + 16); the piece spans nv = (dm + Lc + 15) / 16 vectors, a chunk is
//     HX_FILE_CHUNK / 16 of them, and a workgroup whose chunk starts at or beyond nv leaves.  Chunks partition the vectors of
//     a piece, and images of different slots share no vector: no two workgroups touch the same destination vector;
//   - the row side: vector j's bytes start at row + 16 j - dm, whose misalignment mis is workgroup-uniform; they come from the
//     aligned blocks blk[j] and (mis != 0) blk[j + 1], funnelled into place (v_alignbyte_b32, as k_dense_gather and
//     k_pcm_spread do).  A block is loaded only if it holds a byte of [row, row + Lc): the first vector's low block and the
//     last vector's high block may hold none;
//   - a vector that lies inside [at, at + Lc) in whole is one dwordx4 store; the first and the last vector of a piece may be
//     partial and are stored byte by byte, the bytes of the piece only.  Nothing in front of `at` (so nothing of the tag's
//     bytes [0, head_bytes)), nothing at or beyond at + Lc <= cap is written;
//   - the chunk-0 workgroup's first lane writes image_bytes = min(bytes, cap - head_bytes) and, when the piece was cut, sets
//     status bit 64.  No other workgroup reads or writes that word.
// All of a chunk's loads precede its stores.  No LDS, no scratch, no atomics but the status bit.
#include "hx_dev.h"
#include "../../include/hmp3_amd.h"

static_assert(HX_FILE_CHUNK % (16 * 256) == 0, "a chunk is whole steps of 256 lanes x 16 bytes");
#define HX_FILE_STEPS (HX_FILE_CHUNK / 16 / 256)
static_assert(sizeof(HX_LEDGER_BRIEF) == 32, "k_ledger_brief writes a brief as two 16-byte vectors");

// led [S]: the records behind the call's k_ledger; fw [S]; out / out_stride: the call's rows; nfr [S] or null: its counts
__global__ __launch_bounds__(256) void k_file_append(const HX_LEDGER *__restrict__ led, uint2 *__restrict__ fw, unsigned char *__restrict__ img,
                                                     long long pitch, long long cap, const unsigned char *__restrict__ out, long long out_stride,
                                                     const int *__restrict__ nfr, int nframes, int chunks, int *__restrict__ status)
{
    const int s = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const int n = min(nfr ? nfr[s] : nframes, nframes);
    if (n <= 0) return;
    if (!fw[s].y) return;
    const HX_LEDGER *r = led + s;
    const long long L = r->call_bytes;
    if (!r->open || L <= 0) return;
    // (k_ledger leaves a live record alone whose seek-point state this library cannot have written: its call_bytes is the
    // previous call's then, and is not appended again)
    if (!r->ended && ((unsigned) r->npt >= (unsigned) HX_LEDGER_KEPT || r->every < 1)) return;
    const long long bytes = r->bytes, head = r->head_bytes;
    if (bytes < L || head < 0) return;          // (a record this library cannot have written)
    const long long at = head + bytes - L;
    const long long Lc = min(L, cap - at);
    if (c == 0 && threadIdx.x == 0) {
        fw[s].x = (unsigned) max(0LL, min(bytes, cap - head));
        if (Lc < L) atomicOr(status, 64);
    }
    if (Lc <= 0) return;
    const unsigned dm = (unsigned) (at & 15);
    const long long nv = ((long long) dm + Lc + 15) >> 4;
    if ((long long) c * (HX_FILE_CHUNK / 16) >= nv) return;
    const unsigned char *row = out + (long long) s * out_stride;
    unsigned char *dbase = img + (long long) s * pitch + (at - dm);        // vector 0 of the piece: 16-byte aligned
    const unsigned char *sv = row - dm;                                     // where vector 0's bytes would start on the row side
    const unsigned mis = (unsigned) (reinterpret_cast<unsigned long long>(sv) & 15u), ws = mis >> 2, sh = mis & 3;
    const unsigned char *bbase = sv - mis;                                  // block 0
    const long long v0 = (long long) c * (HX_FILE_CHUNK / 16) + (long long) threadIdx.x;
    // block k holds row bytes [16 k - dm - mis, + 16): one of the piece's when that range meets [0, Lc)
    const long long shift = (long long) dm + mis;
    uint4 lo[HX_FILE_STEPS], hi[HX_FILE_STEPS];
#pragma unroll
    for (int k = 0; k < HX_FILE_STEPS; k++) {
        const long long v = v0 + 256 * k;
        lo[k] = hi[k] = make_uint4(0, 0, 0, 0);
        if (v < nv) {
            const long long b0 = 16 * v - shift;           // row offset of block v's first byte
            if (b0 + 16 > 0 && b0 < Lc) lo[k] = reinterpret_cast<const uint4 *>(bbase)[v];
            if (mis && b0 + 32 > 0 && b0 + 16 < Lc) hi[k] = reinterpret_cast<const uint4 *>(bbase)[v + 1];
        }
    }
#pragma unroll
    for (int k = 0; k < HX_FILE_STEPS; k++) {
        const long long v = v0 + 256 * k;
        if (v >= nv) break;
        uint4 val = lo[k];
        if (mis) {
            unsigned q[8] = {lo[k].x, lo[k].y, lo[k].z, lo[k].w, hi[k].x, hi[k].y, hi[k].z, hi[k].w};
            if (ws & 2) {
#pragma unroll
                for (int j = 0; j < 6; j++) q[j] = q[j + 2];
            }
            if (ws & 1) {
#pragma unroll
                for (int j = 0; j < 5; j++) q[j] = q[j + 1];
            }
            val.x = __builtin_amdgcn_alignbyte(q[1], q[0], sh);
            val.y = __builtin_amdgcn_alignbyte(q[2], q[1], sh);
            val.z = __builtin_amdgcn_alignbyte(q[3], q[2], sh);
            val.w = __builtin_amdgcn_alignbyte(q[4], q[3], sh);
        }
        // the vector's bytes [first, last) are the piece's: row offsets 16 v - dm + i, 0 <= ... < Lc
        const long long o = 16 * v - dm;
        const int first = (int) max(0LL, -o), last = (int) min(16LL, Lc - o);
        unsigned char *d = dbase + 16 * v;
        if (first == 0 && last == 16) *reinterpret_cast<uint4 *>(d) = val;
        else {
            const unsigned w[4] = {val.x, val.y, val.z, val.w};
#pragma unroll
            for (int i = 0; i < 16; i++)
                if (i >= first && i < last) d[i] = (unsigned char) (w[i >> 2] >> (8 * (i & 3)));
        }
    }
}

// the slots hx_batch_ledger_begin opens: image_bytes = 0, and whether the record has an image (on: images are on now)
__global__ __launch_bounds__(256) void k_file_begin(uint2 *__restrict__ fw, const HxLedgerEntry *__restrict__ ent, int n, unsigned on)
{
    const int e = (int) (blockIdx.x * 256 + threadIdx.x);
    if (e < n) fw[ent[e].slot] = make_uint2(0u, on);
}

// out[s] = hx_ledger_brief(led[s], fw[s].x) for every slot; led null (no ledger yet): closed records; fw null: no image words
__global__ __launch_bounds__(256) void k_ledger_brief(const HX_LEDGER *__restrict__ led, const uint2 *__restrict__ fw, HX_LEDGER_BRIEF *__restrict__ out, int S)
{
    const int s = (int) (blockIdx.x * 256 + threadIdx.x);
    if (s >= S) return;
    uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
    if (led) {
        const HX_LEDGER *r = led + s;
        a = make_uint4((unsigned) r->open, (unsigned) r->ended, (unsigned) r->fed, r->frames);
        b = make_uint4(r->bytes, r->crc, (unsigned) r->call_bytes, 0u);
    }
    if (fw) b.w = fw[s].x;
    uint4 *d = reinterpret_cast<uint4 *>(out + s);
    d[0] = a;
    d[1] = b;
}

// ---- finished files (include/hmp3_amd.h, "finished files"): the tag frame, and the fetch of many ----
// k_file_tag: one workgroup per listed slot builds hx_file_tag_build(record, tag) (hx_xhead.cpp: hx_xing_header,
// hx_xing_load_points, hx_xing_update_info) in LDS and stores it once into image bytes [0, head_bytes).
//   - every lane derives the frame's shape as hx_xing_header does - the effective flags (a CBR file below 64 kbit/s loses its
//     TOC), the frame's size, the fields' places - and the trimmed frame count as hx_xing_update_info does: workgroup-uniform
//     scalars.  A workgroup leaves before it writes anything when the record has no image, when the size is not the record's
//     head_bytes (or 0, or beyond cap), or when the record's point state is out of range: where the host function returns 0;
//   - the lanes zero the frame and copy the record's points into LDS; lane 0 writes the header, the counts and the LAME
//     fields; lane i < 100 writes TOC byte i: the points are non-decreasing in frames, so the point build_toc's monotone walk
//     stops at for target i * frames is the first one above it, found by bisection, the file's end standing behind the last
//     point; the interpolation is build_toc's, operation for operation in double (the unit is built with -ffp-contract=off);
//   - the tag CRC: lane w of the first wave takes the seed-0 CRC of bytes [4 w, 4 w + 4) of the frame up to the CRC's place
//     (at most 230 bytes) and shifts it over the bytes behind them (ledger_combine: CRC * x^(8 n)); the XOR of all is the CRC;
//   - the store: a vector that lies in [0, head_bytes) in whole is one dwordx4 store (an image starts 16-byte aligned), the
//     last one goes byte by byte: the audio starts at head_bytes at any residue, and nothing at or beyond it is written.
// The record, the length words and every other byte of the images are only read.
static_assert(sizeof(HX_FILE_TAG) == sizeof(HxFileTagEntry::tag) && HX_FILE_TAG_MAX % 16 == 0, "a tag entry carries an HX_FILE_TAG; the frame is stored as vectors");
__device__ const int file_tag_kbps[2][16] = {{0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 0},
                                             {0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 0}};

__global__ __launch_bounds__(256) void k_file_tag(const HX_LEDGER *__restrict__ led, const uint2 *__restrict__ fw, unsigned char *__restrict__ img,
                                                  long long pitch, long long cap, const HxFileTagEntry *__restrict__ ent)
{
    __shared__ uint4 framev[HX_FILE_TAG_MAX / 16];
    __shared__ int2 pts[HX_LEDGER_KEPT];
    __shared__ unsigned part[HX_WAVE];
    const int tid = (int) threadIdx.x;
    const HxFileTagEntry *en = ent + blockIdx.x;
    const int s = en->slot;
    const HX_FILE_TAG t = *reinterpret_cast<const HX_FILE_TAG *>(en->tag);
    const HX_LEDGER *r = led + s;
    if (!fw[s].y) return;
    const int head = r->head_bytes, npt = r->npt;
    if (head <= 0 || head > cap || head > HX_FILE_TAG_MAX || (unsigned) npt >= (unsigned) HX_LEDGER_KEPT || r->every < 1) return;
    // the frame's shape (hx_xing_header)
    const int h_mode = t.h_mode & 3;
    int flags = t.flags & 127;
    int sri = t.samprate == 22050 ? 0 : t.samprate == 24000 ? 1 : t.samprate == 16000 ? 2 : t.samprate == 44100 ? 3 : t.samprate == 48000 ? 4 : t.samprate == 32000 ? 5 : 6;
    if (sri >= 6) return;
    const int mpeg1 = sri >= 3;
    if (mpeg1) sri -= 3;
    const int side = mpeg1 ? (h_mode == 3 ? 17 : 32) : (h_mode == 3 ? 9 : 17);
    const bool cbr = t.vbr_scale == -1;
    int bri_cbr = 0;
    for (int i = 1; i < 15; i++) if (!bri_cbr && file_tag_kbps[mpeg1][i] == t.kbps) bri_cbr = i;
    if (cbr && file_tag_kbps[mpeg1][bri_cbr] < 64) flags &= ~4;
    const int need = 4 + side + 8 + ((flags & 1) ? 4 : 0) + ((flags & 2) ? 4 : 0) + ((flags & 4) ? 100 : 0) + ((flags & 8) ? 4 : 0) +
                     ((flags & 16) ? 20 : 0) + ((flags & 32) ? 20 : 0) + ((flags & 64) ? 36 : 0);
    const int div = mpeg1 ? t.samprate : 2 * t.samprate;
    int bri = bri_cbr, size = 0;
    if (!cbr) {
        for (bri = 1; bri < 15; bri++) { size = 144000 * file_tag_kbps[mpeg1][bri] / div; if (size >= need) break; }
        if (bri >= 15) return;
    } else {
        size = 144000 * file_tag_kbps[mpeg1][bri_cbr] / div;
        if (size < need) return;
    }
    if (size != head) return;
    // the counts (hx_xing_update_info): the frame count is trimmed where the 12-bit padding field would overflow - also when
    // the audio is longer than the frames, since the unsigned difference wraps
    unsigned frames = r->frames;
    const unsigned nbytes = (unsigned) head + r->bytes;
    unsigned in_sr = t.in_samplerate, out_sr = (unsigned) t.samprate;
    if (in_sr == 0 || out_sr == 0) in_sr = out_sr = 1;
    const unsigned spf = mpeg1 ? 1152u : 576u;
    int pad_end = 0;
    if (t.samples_audio > 0) {
        const unsigned long long audio_r = (unsigned long long) ((double) t.samples_audio * ((double) out_sr / (double) in_sr) + 0.5);
        unsigned long long mp3 = (unsigned long long) frames * spf;
        if (mp3 - audio_r - 1680ull >= 4096ull) {
            frames = (unsigned) ((audio_r + 1680ull + 1152ull) / spf);
            mp3 = frames * spf;                         // (32-bit product, as on the host)
        }
        pad_end = (int) ((long long) (mp3 - audio_r)) - 1680;
    }
    // the fields' places
    int p = 4 + side + 8;
    const int frames_at = p; p += (flags & 1) ? 4 : 0;
    const int bytes_at = p;  p += (flags & 2) ? 4 : 0;
    const int toc_at = p;    p += (flags & 4) ? 100 : 0;
    const int scale_at = p;  p += (flags & 8) ? 4 : 0;
    p += ((flags & 16) ? 20 : 0) + ((flags & 32) ? 20 : 0);
    const int info_at = p;
    const bool info = (flags & 64) && t.samples_audio != 0;

    for (int i = tid; i < HX_FILE_TAG_MAX / 16; i += 256) framev[i] = make_uint4(0, 0, 0, 0);
    const int2 *rp = reinterpret_cast<const int2 *>(&r->pt[0][0]);
    for (int i = tid; i < npt; i += 256) pts[i] = rp[i];
    __syncthreads();
    unsigned char *frame = reinterpret_cast<unsigned char *>(framev);
    auto be32 = [&](int at, unsigned v) { frame[at] = (unsigned char) (v >> 24); frame[at + 1] = (unsigned char) (v >> 16); frame[at + 2] = (unsigned char) (v >> 8); frame[at + 3] = (unsigned char) v; };
    if (tid == 0) {
        frame[0] = 0xFF;
        frame[1] = (unsigned char) (0xF3 | (mpeg1 << 3));
        frame[2] = (unsigned char) ((bri << 4) | (sri << 2));
        frame[3] = (unsigned char) ((h_mode << 6) | ((t.cr_bit & 1) << 3) | ((t.original_bit & 1) << 2));
        be32(4 + side, cbr ? 0x496E666Fu : 0x58696E67u);        // "Info" : "Xing"
        be32(4 + side + 4, (unsigned) flags);
        if (flags & 1) be32(frames_at, frames);
        if (flags & 2) be32(bytes_at, nbytes);
        if (flags & 8) be32(scale_at, (unsigned) t.vbr_scale);
        if (info) {
            const unsigned char lame[9] = {'L', 'A', 'M', 'E', 'H', '5', '.', '2', '4'};
#pragma unroll
            for (int i = 0; i < 9; i++) frame[info_at + i] = lame[i];
            frame[info_at + 9] = (unsigned char) (cbr ? 1 : 0);
            frame[info_at + 10] = (unsigned char) ((t.lowpass / 100) & 0xFF);
            // (+11 .. +20: ReplayGain peak and gains, encoding flags, bitrate: 0)
            frame[info_at + 21] = (unsigned char) ((1680 >> 4) & 0xFF);
            frame[info_at + 22] = (unsigned char) (((1680 << 4) & 0xF0) | ((pad_end >> 8) & 0x0F));
            frame[info_at + 23] = (unsigned char) (pad_end & 0xFF);
            frame[info_at + 24] = (unsigned char) (0x1C | (in_sr == 44100 ? 0x40 : in_sr == 48000 ? 0x80 : in_sr > 48000 ? 0xC0 : 0));
            // (+25 .. +27: MP3 gain, preset, surround: 0)
            be32(info_at + 28, nbytes);
            frame[info_at + 32] = (unsigned char) (r->crc >> 8);
            frame[info_at + 33] = (unsigned char) r->crc;
        }
    }
    const int tot_frames = (int) frames, tot_bytes = (int) nbytes;
    if ((flags & 4) && tid < 100 && tot_frames > 0 && tot_bytes > 0) {
        const int target = tid * tot_frames;
        int lo = 0, hi = npt;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (pts[mid].x * 100 <= target) lo = mid + 1; else hi = mid;
        }
        int f0 = 0, b0 = 0, f1 = tot_frames * 100, b1 = tot_bytes;
        if (lo > 0) { const int2 q = pts[lo - 1]; f0 = q.x * 100; b0 = q.y; }
        if (lo < npt) { const int2 q = pts[lo]; f1 = q.x * 100; b1 = q.y; }
        const double a = 256.0 / tot_bytes;
        const double b = b0 + ((double) (target - f0)) * ((double) (b1 - b0)) / ((double) (f1 - f0));
        int v = (int) (a * b + 0.5);
        v = v < 0 ? 0 : v > 255 ? 255 : v;
        frame[toc_at + tid] = (unsigned char) v;
    }
    __syncthreads();
    // the tag CRC over frame[0, L)
    const int L = info_at + 34;
    if (info && tid < HX_WAVE) {
        unsigned c = 0;
        const int from = 4 * tid, to = min(L, from + 4);
        for (int i = from; i < to; i++) c = crc_byte(c, frame[i]);
        part[tid] = to > from ? ledger_combine(c, 0u, (unsigned) (L - to)) : 0u;
    }
    __syncthreads();
    if (info && tid == 0) {
        unsigned c = 0;
        for (int i = 0; i < HX_WAVE; i++) c ^= part[i];
        frame[L] = (unsigned char) (c >> 8);
        frame[L + 1] = (unsigned char) c;
    }
    __syncthreads();
    unsigned char *dst = img + (long long) s * pitch;
    for (int j = tid; 16 * j < head; j += 256) {
        if (16 * j + 16 <= head) reinterpret_cast<uint4 *>(dst)[j] = framev[j];
        else for (int i = 16 * j; i < head; i++) dst[i] = frame[i];
    }
}
static_assert(4 + 32 + 8 + 4 + 4 + 100 + 4 + 20 + 20 + 34 <= 4 * HX_WAVE, "one wave's lanes, four bytes each, cover the bytes under the tag CRC");

// The fetch of many files: segment e of the image is slot ent[e].slot's first len_e = head_bytes + image_bytes bytes (the
// device's own words; never more than cap), at off[e] = sum over j < e of len_j rounded up to 16, zeros up to off[e + 1].
__device__ __forceinline__ long long file_len(const HX_LEDGER *led, const uint2 *fw, int s, long long cap)
{
    const long long head = led ? (long long) max(led[s].head_bytes, 0) : 0;
    return min(head + (long long) fw[s].x, cap);
}
// The offsets: k_dense_off's exclusive scan, over the list.  off [n + 1]; status bit 16: the image does not fit dst_cap (the
// offsets are complete all the same)
__global__ __launch_bounds__(1024) void k_file_off(const HxLedgerEntry *__restrict__ ent, int n, const HX_LEDGER *__restrict__ led, const uint2 *__restrict__ fw,
                                                   long long cap, long long *__restrict__ off, long long dst_cap, int *__restrict__ status)
{
    __shared__ long long wsum[16];
    const int tid = (int) threadIdx.x, lane = tid & 63, w = tid >> 6;
    long long base = 0;         // 16-byte units in front of this round
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        const long long v = (i < n) ? (file_len(led, fw, ent[i].slot, cap) + 15) >> 4 : 0;
        const long long incl = ((long long) hx_wave_scan((int) (v >> 32)) << 32) + ((long long) hx_wave_scan((int) ((v >> 16) & 0xFFFF)) << 16) + hx_wave_scan((int) (v & 0xFFFF));
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        long long before = 0, all = 0;
        for (int k = 0; k < 16; k++) { const long long x = wsum[k]; all += x; before += (k < w) ? x : 0; }
        if (i < n) off[i] = (base + before + incl - v) << 4;
        base += all;
        __syncthreads();        // wsum is rewritten by the next round
    }
    if (tid == 0) {
        off[n] = base << 4;
        if ((base << 4) > dst_cap) atomicOr(status, 16);
    }
}
// The gather: workgroup (entry e, chunk c) moves bytes [c * HX_FILE_GATHER_CHUNK, ...) of the listed image, 16 per lane and
// step; the host does not know the lengths, so the grid covers the images' pitch and a workgroup past its segment leaves at
// once.  Both sides are 16-byte aligned - an image starts so, off is a multiple of 16 - so every access is a dwordx4, a
// chunk's loads ahead of its stores.  A segment's last vector carries its zero padding; its load stays inside the slot's
// pitch (len <= cap <= pitch, a multiple of 16).  A segment that does not fit below dst_cap in whole is not written.
static_assert(HX_FILE_GATHER_CHUNK % (16 * 256) == 0, "a chunk is whole steps of 256 lanes x 16 bytes");
#define HX_FILE_GATHER_STEPS (HX_FILE_GATHER_CHUNK / 16 / 256)
__global__ __launch_bounds__(256) void k_file_gather(const HxLedgerEntry *__restrict__ ent, const HX_LEDGER *__restrict__ led, const uint2 *__restrict__ fw,
                                                     const unsigned char *__restrict__ img, long long pitch, long long cap, const long long *__restrict__ off,
                                                     unsigned char *__restrict__ dst, long long dst_cap, int chunks)
{
    const int e = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const int s = ent[e].slot;
    const long long len = file_len(led, fw, s, cap);
    if ((long long) c * HX_FILE_GATHER_CHUNK >= len) return;
    if (off[e + 1] > dst_cap) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(img + (long long) s * pitch);
    uint4 *d = reinterpret_cast<uint4 *>(dst + off[e]);
    const long long nv = (len + 15) >> 4, v0 = (long long) c * (HX_FILE_GATHER_CHUNK / 16) + (long long) threadIdx.x;
    uint4 val[HX_FILE_GATHER_STEPS];
#pragma unroll
    for (int k = 0; k < HX_FILE_GATHER_STEPS; k++) {
        const long long v = v0 + 256 * k;
        val[k] = v < nv ? src[v] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < HX_FILE_GATHER_STEPS; k++) {
        const long long v = v0 + 256 * k;
        if (v >= nv) break;
        const int rem = (int) min(16LL, len - 16 * v);      // bytes of the file in this vector: the rest is padding
        uint4 x = val[k];
        if (rem < 16) {
            auto keep = [&](unsigned q, int r) { return r >= 4 ? q : (r <= 0 ? 0u : q & ((1u << (8 * r)) - 1u)); };
            x.x = keep(x.x, rem); x.y = keep(x.y, rem - 4); x.z = keep(x.z, rem - 8); x.w = keep(x.w, rem - 12);
        }
        d[v] = x;
    }
}
