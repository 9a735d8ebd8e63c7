// hx_fileimg.hip - file images (include/hmp3_amd.h, "file images"): k_file_append puts the bytes of a call that the ledger gave
// to a file behind the file's bytes so far, in the slot's image; k_file_begin restarts a slot's length word; k_ledger_brief
// writes the short form of every record.  Built as part of hx_pack.hip's unit, behind hx_pcmin.hip.
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
