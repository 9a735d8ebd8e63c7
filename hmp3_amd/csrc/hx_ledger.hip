// hx_ledger.hip - K10: the file ledger (include/hmp3_amd.h, HX_LEDGER): k_ledger updates every stream's record from a call's
// frame counters, per-frame CRCs and byte counts, right behind k_crc; k_ledger_begin opens records, k_ledger_gather copies
// listed records out.  Built as part of hx_pack.hip's unit, behind hx_crc.hip (whose crc_xtimes it uses).
//
// k_ledger: one wave per stream, four streams per 256-lane workgroup, no workgroup barrier, no LDS, no atomics.  The update
// rule is hx_ledger_update's (hx_xhead.cpp), which the tests hold it to bytewise; what differs is the order of work:
//   - the lanes take the stream's counter pairs 64 frames a round (8-byte loads; a counter buffer that starts off an 8-byte
//     boundary is read in 4-byte halves) and find the frame at which the drain ends with a ballot: the first frame f with
//     fed + f >= ncalls - 1 whose frame counter has reached ncalls * frames_per_call;
//   - seek points: frame f of an input call is a point when the countdown toc_counter runs out there, so the points of a
//     round are the frames next, next + every, ... - the lanes that hold them store them side by side, as many as fit under
//     HX_LEDGER_KEPT, and the walk jumps on; a full table is halved by all lanes (point 2i + 1 becomes point i) and `every`
//     doubles, as hx_xing_toc does it;
//   - lane 0 joins the CRC: crc * x^(8 e) ^ c[f], x^(8 e) by square-and-multiply over the bits of e, and writes the state words.
// A wave of a record that is not open, or of a stream that takes no frame, leaves at once; of an ended record it writes
// call_bytes = 0.  What a wave may touch: its own record, and of the call's buffers stats[s][f < n], crc[s][f < n] and
// out_bytes[s] - read only.  Points are stored at indices below HX_LEDGER_KEPT only (a record whose npt / every this library
// cannot have written is left alone).
// The halving reads points that lanes of the same wave stored earlier in the launch: the fence in front of it waits for
// those stores (one CU, one L1: workgroup scope is enough).  Its own loads all precede its stores, and a second fence keeps
// it so in the memory system.
#include "hx_dev.h"
#include "../../include/hmp3_amd.h"

static_assert(sizeof(HX_LEDGER) % 16 == 0 && offsetof(HX_LEDGER, pt) == 4 * HX_LEDGER_HDR_WORDS && HX_LEDGER_POINTS == HX_LEDGER_KEPT + 1,
              "the kernels move records as 16-byte vectors and read the header as HX_LEDGER_HDR_WORDS words");
static_assert(HX_LEDGER_KEPT == 8 * HX_WAVE, "a halving moves four points per lane");
#define HX_LEDGER_VECS ((int) (sizeof(HX_LEDGER) / 16))

// a * b mod P in the CRC register's bit order (hx_crc.hip)
__device__ __forceinline__ unsigned ledger_mulmod(unsigned a, unsigned b)
{
    unsigned r = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) { r ^= b & (0u - ((a >> (15 - i)) & 1u)); b = crc_xtimes(b); }
    return r;
}
// hx_xing_crc_combine: the CRC of A ++ B from the CRCs of A and B and len = |B|
__device__ __forceinline__ unsigned ledger_combine(unsigned crc_a, unsigned crc_b, unsigned len)
{
    unsigned p = 0x8000u, sq = 0x0080u;     // 1, x^8
#pragma unroll 1
    for (; len; len >>= 1) {
        if (len & 1u) p = ledger_mulmod(p, sq);
        sq = ledger_mulmod(sq, sq);
    }
    return (ledger_mulmod(crc_a, p) ^ crc_b) & 0xFFFFu;
}

// frame f's counter pair: one 8-byte load where the caller's buffer allows it (pair: it starts on an 8-byte boundary)
__device__ __forceinline__ int2 ledger_pair(const int *st, int f, bool pair)
{
    return pair ? reinterpret_cast<const int2 *>(st)[f] : make_int2(st[2 * f], st[2 * f + 1]);
}

// led [S]; stats [S][nframes][2], crc [S][nframes], out_bytes [S]: the call's; nfr: [S] its per-stream counts or null
__global__ __launch_bounds__(256) void k_ledger(HX_LEDGER *__restrict__ led, const int *__restrict__ stats, const unsigned short *__restrict__ crc,
                                                const int *__restrict__ out_bytes, const int *__restrict__ nfr, int nframes, int S)
{
    const int lane = (int) threadIdx.x & (HX_WAVE - 1);
    const int s = (int) blockIdx.x * 4 + ((int) threadIdx.x >> 6);
    if (s >= S) return;
    HX_LEDGER *r = led + s;
    const int n = __builtin_amdgcn_readfirstlane(min(nfr ? nfr[s] : nframes, nframes));
    const int hw = lane < HX_LEDGER_HDR_WORDS ? reinterpret_cast<const int *>(r)[lane] : 0;
#define LEDGER_WORD(field) __builtin_amdgcn_readlane(hw, (int) (offsetof(HX_LEDGER, field) / 4))
    const int ncalls = LEDGER_WORD(ncalls), head = LEDGER_WORD(head_bytes), flags = LEDGER_WORD(flags), fed = LEDGER_WORD(fed);
    const int toc = LEDGER_WORD(toc_counter);
    int npt = LEDGER_WORD(npt), every = LEDGER_WORD(every);
    if (!LEDGER_WORD(open) || n <= 0) return;
    if (LEDGER_WORD(ended)) { if (lane == 0) r->call_bytes = 0; return; }
    if (!stats || !crc || (unsigned) npt >= (unsigned) HX_LEDGER_KEPT || every < 1) return;
    const unsigned expected = (unsigned) ncalls * (unsigned) LEDGER_WORD(frames_per_call), crc0 = (unsigned) LEDGER_WORD(crc);
#undef LEDGER_WORD
    const int *st = stats + (long long) s * nframes * 2;
    const bool pair = (reinterpret_cast<unsigned long long>(stats) & 7ull) == 0;
    int2 *pt = reinterpret_cast<int2 *>(&r->pt[0][0]);
    const int tocn = (flags & 1) ? max(0, min(n, ncalls - fed)) : 0;    // the call's frames that are input calls of a file with seek points
    int next = toc <= 1 ? 0 : toc - 1;          // the frame of the next point
    int lastp = -1, fe = -1, walked = 0;        // the last point's frame; the end frame; frames the countdown has seen
    for (int base = 0; base < n && fe < 0; base += HX_WAVE) {
        const int f = base + lane;
        const int2 v = f < n ? ledger_pair(st, f, pair) : make_int2(0, 0);
        const unsigned long long m = __ballot(f < n && fed + f >= ncalls - 1 && (unsigned) v.x >= expected);
        if (m) fe = base + __ffsll((long long) m) - 1;
        const int lim = min(tocn, fe >= 0 ? fe + 1 : min(n, base + HX_WAVE));
        while (next < lim) {
            const int k = min((lim - 1 - next) / every + 1, HX_LEDGER_KEPT - npt);      // points of this round that fit
            const int d = f - next, j = d / every;
            if (d >= 0 && j < k && j * every == d) pt[npt + j] = make_int2(v.x + 1, v.y + head);
            npt += k;
            lastp = next + (k - 1) * every;
            if (npt == HX_LEDGER_KEPT) {
                __threadfence_block();
                int2 kp[4];
#pragma unroll
                for (int q = 0; q < 4; q++) kp[q] = pt[2 * (lane + HX_WAVE * q) + 1];
                __threadfence_block();
#pragma unroll
                for (int q = 0; q < 4; q++) pt[lane + HX_WAVE * q] = kp[q];
                npt = HX_LEDGER_KEPT / 2;
                every += every;
            }
            next = lastp + every;
        }
        walked = max(walked, lim);
    }
    if (lane != 0) return;
    const int fl = fe >= 0 ? fe : n - 1;        // the last frame the file uses of this call
    const int2 v = ledger_pair(st, fl, pair);
    const unsigned e = (unsigned) out_bytes[s] - ((unsigned) st[2 * (n - 1) + 1] - (unsigned) v.y);
    r->frames = (unsigned) v.x;
    r->bytes = (unsigned) v.y;
    r->crc = ledger_combine(crc0, crc[(long long) s * nframes + fl], e);
    r->call_bytes = (int) e;
    r->fed = fed + fl + 1;
    if (fe >= 0) r->ended = 1;
    if (walked > 0) {
        r->toc_counter = lastp >= 0 ? every - (walked - 1 - lastp) : toc - walked;
        r->npt = npt;
        r->every = every;
    }
}

// slot ent[e].slot gets a new open record: the entry's parameters, its frames per call among them (the host's view of the slot
// when the call was made), everything else 0 but every = 1
__global__ __launch_bounds__(256) void k_ledger_begin(HX_LEDGER *__restrict__ led, const HxLedgerEntry *__restrict__ ent)
{
    const HxLedgerEntry en = ent[blockIdx.x];
    uint4 *dst = reinterpret_cast<uint4 *>(led + en.slot);
    for (int w = (int) threadIdx.x; w < HX_LEDGER_VECS; w += 256) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (w == 0) v = make_uint4((unsigned) en.ncalls, (unsigned) en.fpc, (unsigned) en.head_bytes, (unsigned) en.flags);
        else if (w == (int) (offsetof(HX_LEDGER, open) / 16)) v.x = 1;
        else if (w == (int) (offsetof(HX_LEDGER, every) / 16)) v.y = 1;
        dst[w] = v;
    }
}
static_assert(offsetof(HX_LEDGER, open) == 16 && offsetof(HX_LEDGER, every) == 52 && offsetof(HX_LEDGER, flags) == 12, "k_ledger_begin writes the header as four vectors");

// out[e] = the record of slot ent[e].slot
__global__ __launch_bounds__(256) void k_ledger_gather(const HX_LEDGER *__restrict__ led, const HxLedgerEntry *__restrict__ ent, HX_LEDGER *__restrict__ out)
{
    const uint4 *src = reinterpret_cast<const uint4 *>(led + ent[blockIdx.x].slot);
    uint4 *dst = reinterpret_cast<uint4 *>(out + blockIdx.x);
    for (int w = (int) threadIdx.x; w < HX_LEDGER_VECS; w += 256) dst[w] = src[w];
}
