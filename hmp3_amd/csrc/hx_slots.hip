// hx_slots.hip - K9: slot operations on one or many streams of a batch in one launch (hx_batch_slots.hip: every reset, save
// and restore): k_slot_reset, k_slot_gather, k_slot_scatter.  Built as part of hx_pack.hip's unit.
//
// Pure data movers, no LDS.  Grid (entry, chunk): workgroup e * chunks + c handles 8-byte words [c * HX_SLOT_CHUNK, ...) of
// entry e, HX_SLOT_VEC words per lane, all loads of a lane issued before its stores.  The unit is the 8-byte word (dwordx2):
// HxStream sits sizeof(HxStateHeader) = 24 bytes into a blob whose base is 16-byte aligned, so the blob side of every copy is
// 8-byte aligned and no more, while the batch side (d_st rows, subband rows, converter carry) is 16-byte aligned.  With
// dwordx2 both sides are aligned as they stand and a wave still covers 512 contiguous bytes per instruction; the other
// choice - dwordx4 on the batch side, two aligned vectors funnelled on the blob side as k_dense_gather does - halves the
// instructions on one side and adds the funnel's moves for a copy of 39 KB per stream that the call's launch dominates.
// What a kernel may touch: the listed slots' HxStream, slots 0..2 of their subband rows, their converter words, and bytes
// [0, n * blob_stride) of the blob array.  The host has checked that every slot is in range and listed once.
#include "hx_dev.h"

static_assert(sizeof(HxSlotEntry) == 24, "the host stages the entries as 24-byte records");
static_assert(HX_SLOT_SRC_WORD == HX_SLOT_ST_WORDS + 2 * HX_SLOT_CARRY_WORDS, "slot_word walks the parts in the blob's order (hx_types.h)");

__device__ __forceinline__ uint2 slot_split(unsigned long long v) { return make_uint2((unsigned) v, (unsigned) (v >> 32)); }
__device__ __forceinline__ unsigned long long slot_join(uint2 v) { return (unsigned long long) v.x | ((unsigned long long) v.y << 32); }

// Where word w of a slot's state lives in the batch, w counted from the start of HxStream: the stream record, the carry of
// channel 0 and 1, the converter's carried samples (the copy the next call reads).  Null: not a word of the batch (the
// converter's fingerprint and call count, which the callers place themselves, and the padding).
__device__ __forceinline__ uint2 *slot_word(const SlotArgs &a, int slot, int w)
{
    if (w < HX_SLOT_ST_WORDS) return reinterpret_cast<uint2 *>(a.st + slot) + w;
    w -= HX_SLOT_ST_WORDS;
    if (w < 2 * HX_SLOT_CARRY_WORDS) {
        const int ch = w >= HX_SLOT_CARRY_WORDS;
        return reinterpret_cast<uint2 *>(a.sb + ((long long) slot * 2 + ch) * a.sb_row) + (w - ch * HX_SLOT_CARRY_WORDS);
    }
    w -= HX_SLOT_SRC_CARRY_WORD - HX_SLOT_ST_WORDS;
    if (a.src_calls && w >= 0 && w < HX_SLOT_SRC_CARRY_WORDS)
        return reinterpret_cast<uint2 *>(a.src_carry + ((long long) a.src_par * a.S + slot) * 2 * HX_SRC_CARRY) + w;
    return nullptr;
}

// Every listed slot becomes a new stream of its entry's class: the class's initial HxStream, a zero subband carry and
// (converting batches) zero call counts in both copies, the entry's plan in the slot's word of src_cls and that plan's
// fingerprint in its word of src_fp - the same values as before when the slot keeps its configuration - and, where the batch
// has one, a zero decoded-PCM state.  The converter's
// carried samples stay: call 0 of any plan reads none (hx_src.hip: qstart(0) = u(0) = 0).  Only slots 0..2 of the two subband rows are zeroed: k_polyphase writes slots
// 3 .. NG + 2 of a call before k_spec (slots 0 .. NG) and k_msscan (slots NG .. NG + 2) read them, and its own read is of
// slot 2.
__global__ __launch_bounds__(256) void k_slot_reset(SlotArgs a)
{
    const int e = blockIdx.x / a.chunks, c = blockIdx.x - e * a.chunks;
    const HxSlotEntry en = a.ent[e];
    const uint2 *img = reinterpret_cast<const uint2 *>(a.init + en.cls);
    uint2 v[HX_SLOT_VEC];
#pragma unroll
    for (int k = 0; k < HX_SLOT_VEC; k++) {
        const int w = c * HX_SLOT_CHUNK + 256 * k + (int) threadIdx.x;
        v[k] = (w < HX_SLOT_ST_WORDS) ? img[w] : make_uint2(0, 0);
    }
#pragma unroll
    for (int k = 0; k < HX_SLOT_VEC; k++) {
        const int w = c * HX_SLOT_CHUNK + 256 * k + (int) threadIdx.x;
        if (w < HX_SLOT_SRC_WORD) *slot_word(a, en.slot, w) = v[k];
        else if (a.src_calls && w < HX_SLOT_SRC_WORD + 2) a.src_calls[(long long) (w - HX_SLOT_SRC_WORD) * a.S + en.slot] = 0;
        else if (a.src_calls && w == HX_SLOT_SRC_WORD + 2) { a.src_cls[en.slot] = en.plan; a.src_fp[en.slot] = a.plan_fp[en.plan]; }
    }
    // the decoded PCM's carried state (hx_batch_recon_buffer): a new stream's decoder starts from zero; the entry's workgroups share the floats
    if (a.recon_state)
        for (int i = c * 256 + (int) threadIdx.x; i < HX_RECON_STATE_FLOATS; i += a.chunks * 256) a.recon_state[(long long) en.slot * HX_RECON_STATE_FLOATS + i] = 0.0f;
}

// Blob e of blobs [n][blob_words] = the stream-state blob of entry e's slot (layout: hx_types.h), and zeros from the blob's
// end to the stride.
__global__ __launch_bounds__(256) void k_slot_gather(SlotArgs a, uint2 *__restrict__ blobs)
{
    const int e = blockIdx.x / a.chunks, c = blockIdx.x - e * a.chunks;
    const HxSlotEntry en = a.ent[e];
    uint2 *dst = blobs + (long long) e * a.blob_words;
    uint2 v[HX_SLOT_VEC];
#pragma unroll
    for (int k = 0; k < HX_SLOT_VEC; k++) {
        const int w = c * HX_SLOT_CHUNK + 256 * k + (int) threadIdx.x, ws = w - HX_SLOT_HDR_WORDS;
        v[k] = make_uint2(0, 0);
        if (w >= a.blob_words) continue;
        if (w == HX_SLOT_HDR_MAGIC) v[k] = make_uint2(a.magic, a.version);
        else if (w == HX_SLOT_HDR_STATE_BYTES) v[k] = make_uint2((unsigned) sizeof(HxStream), 0);
        else if (w == HX_SLOT_HDR_CFG) v[k] = slot_split(en.cfg);
        else if (const uint2 *p = slot_word(a, en.slot, ws)) v[k] = *p;
        else if (a.src_calls && ws == HX_SLOT_SRC_WORD) v[k] = slot_split(a.src_fp[en.slot]);
        else if (a.src_calls && ws == HX_SLOT_SRC_WORD + 1) v[k] = slot_split((unsigned long long) a.src_calls[(long long) a.src_par * a.S + en.slot]);
    }
#pragma unroll
    for (int k = 0; k < HX_SLOT_VEC; k++) {
        const int w = c * HX_SLOT_CHUNK + 256 * k + (int) threadIdx.x;
        if (w < a.blob_words) dst[w] = v[k];
    }
}

// The reverse.  Every workgroup of an entry checks the blob's header (and, converting batches, the plan fingerprint)
// against what the slot takes; on a mismatch none of them writes anything and status bit 32 is set.  HxStream goes in with
// cls replaced by the entry's (the class index is the receiving batch's), the carry into slots 0..2 of both channels, the
// converter's call count into both copies; where the batch has a decoded-PCM state, the slot's is zeroed.
__global__ __launch_bounds__(256) void k_slot_scatter(SlotArgs a, const uint2 *__restrict__ blobs)
{
    const int e = blockIdx.x / a.chunks, c = blockIdx.x - e * a.chunks;
    const HxSlotEntry en = a.ent[e];
    const uint2 *src = blobs + (long long) e * a.blob_words;
    const uint2 magic_version = src[HX_SLOT_HDR_MAGIC], state_bytes = src[HX_SLOT_HDR_STATE_BYTES], cfg = src[HX_SLOT_HDR_CFG];
    bool ok = magic_version.x == a.magic && magic_version.y == a.version && state_bytes.x == (unsigned) sizeof(HxStream) && slot_join(cfg) == en.cfg;
    if (a.src_calls) ok = ok && slot_join(src[HX_SLOT_HDR_WORDS + HX_SLOT_SRC_WORD]) == a.src_fp[en.slot];
    if (!ok) {
        if (c == 0 && threadIdx.x == 0) atomicOr(a.status, 32);
        return;
    }
    const int nw = a.src_calls ? HX_SLOT_SRC_CARRY_WORD + HX_SLOT_SRC_CARRY_WORDS : HX_SLOT_SRC_WORD;      // words of state behind the header
    uint2 v[HX_SLOT_VEC];
#pragma unroll
    for (int k = 0; k < HX_SLOT_VEC; k++) {
        const int ws = c * HX_SLOT_CHUNK + 256 * k + (int) threadIdx.x;
        v[k] = (ws < nw) ? src[HX_SLOT_HDR_WORDS + ws] : make_uint2(0, 0);
        if (ws == 0) v[k].x = (unsigned) en.cls;
    }
#pragma unroll
    for (int k = 0; k < HX_SLOT_VEC; k++) {
        const int ws = c * HX_SLOT_CHUNK + 256 * k + (int) threadIdx.x;
        if (ws >= nw) continue;
        if (uint2 *p = slot_word(a, en.slot, ws)) *p = v[k];
        else if (ws == HX_SLOT_SRC_WORD + 1) {
            a.src_calls[en.slot] = (long long) slot_join(v[k]);
            a.src_calls[(long long) a.S + en.slot] = (long long) slot_join(v[k]);
        }
    }
    // the decoded PCM's carried state is not part of a blob: a restored stream's decoder starts from zero, whatever the slot
    // ran before (an accepted blob only; the entry's workgroups share the floats)
    if (a.recon_state)
        for (int i = c * 256 + (int) threadIdx.x; i < HX_RECON_STATE_FLOATS; i += a.chunks * 256) a.recon_state[(long long) en.slot * HX_RECON_STATE_FLOATS + i] = 0.0f;
}
