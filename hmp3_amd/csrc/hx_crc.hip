// hx_crc.hip - k_crc: the MusicCRC of a call's bitstreams (hx_batch_crc_buffer), behind the packing.
//
// The value is xhead.c's XingHeaderUpdateCRC (hx_xing_update_crc): CRC-16, reflected, polynomial 0xA001, seed 0, so bit 15
// of the register is the coefficient of x^0 and the register after a message M is M(x) * x^16 mod P.  That makes it linear:
//   CRC(0, A ++ B) = CRC(0, A) * x^(8 |B|) mod P  ^  CRC(0, B)
// (hx_xing_crc_combine is the same identity on the host).  Per stream, one workgroup:
//   1. every lane takes the seed-0 CRC of HX_CRC_CHUNK bytes of the row's used part;
//   2. a scan over the lanes with that combine gives the CRC from the row's start to every chunk's end - step k of it
//      joins runs of 2^k chunks, so its shift x^(8 * HX_CRC_CHUNK * 2^k) is a compile-time constant and the multiplication
//      sixteen AND / XOR pairs on immediates;
//   3. one lane per input frame f takes the CRC at the start of the chunk in which e[f] (include/hmp3_amd.h) ends and
//      extends it over the less than one chunk that is left.
// A row longer than HX_CRC_LANES chunks takes several passes; the CRC at a pass's end seeds lane 0 of the next.
// The byte step is plain ALU - the table entry of CRC-16/ARC in closed form, (x << 6) ^ (x << 7) ^ (parity(x) ? 0xC001 : 0)
// for x = (crc ^ byte) & 0xFF - and not a 256-entry table in LDS: the lookups would be data-dependent, 64 lanes into 32
// banks, while the ALU form is about a dozen instructions a byte and the kernel has the chip to itself.
// Rows carry no alignment promise: the bytes in front of the row's first 16-byte boundary (at most 15) are taken one by
// one and seed the first pass, chunks start on 16-byte boundaries from there and are read as dwordx4 vectors, and only
// vectors that lie inside the used part in whole are read - the bytes behind the last one go one by one in step 3.
// Nothing at or beyond out_bytes[i] of a row is read, and no counter of a frame >= nframes.
#include "hx_dev.h"

#define HX_CRC_CHUNK 64                 // bytes per lane and pass: four vectors
#define HX_CRC_LANES 256
#define HX_CRC_PASS (HX_CRC_CHUNK * HX_CRC_LANES)

// polynomial arithmetic mod P in the register's bit order (bit 15 = x^0): times x, product, x^(8 n)
constexpr unsigned crc_xtimes(unsigned b) { return (b >> 1) ^ ((b & 1u) ? 0xA001u : 0u); }
constexpr unsigned crc_mul(unsigned a, unsigned b)
{
    unsigned r = 0;
    for (int i = 0; i < 16; i++) { if (a & (0x8000u >> i)) r ^= b; b = crc_xtimes(b); }
    return r;
}
constexpr unsigned crc_xpow8(unsigned long long n)
{
    unsigned p = 0x8000u, b = 0x0080u;  // 1, x^8
    for (; n; n >>= 1) { if (n & 1) p = crc_mul(p, b); b = crc_mul(b, b); }
    return p;
}
// a * x^(8 * HX_CRC_CHUNK * 2^K) mod P: what a CRC becomes when 2^K chunks follow
template <int K> __device__ __forceinline__ unsigned crc_shift(unsigned a)
{
    constexpr unsigned x = crc_xpow8((unsigned long long) HX_CRC_CHUNK << K);   // (constexpr: evaluated by the compiler, not by every lane)
    unsigned r = 0, b = x;
#pragma unroll
    for (int i = 0; i < 16; i++) { r ^= b & (0u - ((a >> (15 - i)) & 1u)); b = crc_xtimes(b); }
    return r;
}

// one byte (the low byte of d), four bytes in memory order, a vector
__device__ __forceinline__ unsigned crc_byte(unsigned crc, unsigned d)
{
    const unsigned x = (crc ^ d) & 0xFFu;
    return (crc >> 8) ^ (x << 6) ^ (x << 7) ^ ((0u - (__popc(x) & 1u)) & 0xC001u);
}
__device__ __forceinline__ unsigned crc_word(unsigned crc, unsigned w)
{
    return crc_byte(crc_byte(crc_byte(crc_byte(crc, w), w >> 8), w >> 16), w >> 24);
}
__device__ __forceinline__ unsigned crc_vec(unsigned crc, const uint4 q)
{
    return crc_word(crc_word(crc_word(crc_word(crc, q.x), q.y), q.z), q.w);
}
// len bytes from p on; vec: p is 16-byte aligned
__device__ __forceinline__ unsigned crc_span(unsigned crc, const unsigned char *p, int len, bool vec)
{
    if (vec) for (; len >= 16; len -= 16, p += 16) crc = crc_vec(crc, *reinterpret_cast<const uint4 *>(p));
    for (int k = 0; k < len; k++) crc = crc_byte(crc, p[k]);
    return crc;
}

// step K of the scan: joins the run of 2^K chunks in front (read from sc[K & 1]) and leaves the result in the other half
template <int K> __device__ __forceinline__ unsigned scan_step(unsigned (&sc)[2][HX_CRC_LANES], unsigned v, int tid)
{
    if (tid >= (1 << K)) v ^= crc_shift<K>(sc[K & 1][tid - (1 << K)]);
    sc[(K + 1) & 1][tid] = v;
    __syncthreads();
    return v;
}

// out / out_stride / out_bytes: the call's rows; stats [S][nframes][2]: its frame counters; crc [S][nframes]
__global__ __launch_bounds__(HX_CRC_LANES) void k_crc(const unsigned char *__restrict__ out, long long out_stride, const int *__restrict__ out_bytes,
                                                      const int *__restrict__ stats, int nframes, unsigned short *__restrict__ crc)
{
    __shared__ unsigned sc[2][HX_CRC_LANES];
    const int s = blockIdx.x, tid = threadIdx.x;
    const unsigned char *row = out + (long long) s * out_stride;
    const int nraw = out_bytes[s];
    const int n = (int) min((long long) max(nraw, 0), out_stride);
    const int h = min(n, (int) ((0ull - reinterpret_cast<unsigned long long>(row)) & 15ull));     // bytes in front of the first boundary
    const int *st = stats + (long long) s * nframes * 2;
    unsigned short *dst = crc + (long long) s * nframes;
    const unsigned last = (unsigned) st[2 * (nframes - 1) + 1];
    // e[f], never beyond the used part
    auto emitted = [&](int f) { const unsigned e = (unsigned) nraw - (last - (unsigned) st[2 * f + 1]); return (int) min(e, (unsigned) n); };

    // the frames that end in front of the boundary (e = 0: CRC 0), and the seed of the first pass
    for (int f = tid; f < nframes; f += HX_CRC_LANES) {
        const int e = emitted(f);
        if (e <= h) dst[f] = (unsigned short) crc_span(0, row, e, false);
    }
    unsigned carry = crc_span(0, row, h, false);
    const long long body = (long long) n - h;
    for (long long base = 0; base < body; base += HX_CRC_PASS) {
        // 1. this lane's chunk (whole vectors inside the used part only: a chunk that is cut short is never a prefix)
        const long long o = h + base + (long long) tid * HX_CRC_CHUNK;
        unsigned v = 0;
#pragma unroll
        for (int j = 0; j < HX_CRC_CHUNK / 16; j++)
            if (o + 16 * (j + 1) <= n) v = crc_vec(v, *reinterpret_cast<const uint4 *>(row + o + 16 * j));
        // 2. inclusive scan over the workgroup's lanes (Hillis-Steele through LDS, the two halves of sc in turn): before step
        // K a lane holds the CRC of the 2^K chunks that end with its own - lane 0 the row's CRC up to its chunk's end
        if (tid == 0) v ^= crc_shift<0>(carry);
        sc[0][tid] = v;
        __syncthreads();
        v = scan_step<0>(sc, v, tid); v = scan_step<1>(sc, v, tid); v = scan_step<2>(sc, v, tid); v = scan_step<3>(sc, v, tid);
        v = scan_step<4>(sc, v, tid); v = scan_step<5>(sc, v, tid); v = scan_step<6>(sc, v, tid); v = scan_step<7>(sc, v, tid);
        static_assert(HX_CRC_LANES == 1 << 8, "eight steps scan 256 lanes and leave the result in sc[0]");
        // 3. the frames whose last byte lies in this pass
        for (int f = tid; f < nframes; f += HX_CRC_LANES) {
            const long long q = (long long) emitted(f) - h - 1 - base;      // that byte, counted from the pass's start
            if (q < 0 || q >= HX_CRC_PASS) continue;
            const int c = (int) (q / HX_CRC_CHUNK);
            dst[f] = (unsigned short) crc_span(c ? sc[0][c - 1] : carry, row + h + base + (long long) c * HX_CRC_CHUNK, (int) (q + 1 - (long long) c * HX_CRC_CHUNK), true);
        }
        carry = sc[0][HX_CRC_LANES - 1];
        __syncthreads();        // sc is rewritten by the next pass
    }
}
