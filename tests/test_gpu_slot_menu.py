"""Slot configurations (hx_batch_create_menu, hx_batch_assign_streams, hx_multi_*; kernel: k_slot_reset in
hmp3_amd/csrc/hx_slots.hip): a batch is created over a menu of configurations, and a freed slot takes a stream of any entry.

Shapes are those of test_gpu_slot_ops.py: six slots, max_frames 7, a few frames per call under uneven counts.  The
expectation is one oracle encoder per stream life, fed frame by frame: a slot's life ends at an assign, and the next one
starts a new encoder of the assigned entry's control.  Rows, frame counters and the MusicCRC of every call are compared for
equality; converting batches against the reference's MP3_audio_encode loop where oracle/_ref is built, else against this
library's one-stream encoder."""
import ctypes as C

import numpy as np
import pytest

import packet_cases as PC
from conftest import skip_unless_host_libm_is_the_restated_one
from gpu_support import batch_vs_single_vs_reference, controls, host_crc, ints, oracle_bytes, states, write_wav
from hmp3_amd import api, synth
from oracle import oracle as O
from src_cases import Stream, ref_converted, run

pytestmark = pytest.mark.gpu

S, MAXF = 6, 7
# 44.1 kHz CBR-128 joint stereo, 48 kHz VBR-50, 32 kHz CBR-96 (the odd-partition rate), 44.1 kHz CBR-128 behind the DC blocker
MENU = [dict(bitrate=64), dict(vbr_mnr=50, samprate=48000), dict(bitrate=48, samprate=32000), dict(bitrate=64, filter_select=1)]


def life_pcm(seed, kw, F=24):
    """float32 at int16 scale with non-integral samples and bursts, at the control's rate ([n] for a mono control)"""
    x = synth.stream_pcm(seed, F, sr=kw.get("samprate", 44100), bursts=True)[5 * 1152:].astype(np.float32)
    x += np.random.default_rng(seed).uniform(-0.49, 0.49, x.shape).astype(np.float32)
    return np.ascontiguousarray(x[:, 0] if kw.get("mode") == 3 else x)


class Life:
    """one stream from its first frame: the oracle's frames and how far the stream has come"""

    def __init__(self, seed, kw):
        self.kw, self.pcm = kw, life_pcm(seed, kw)
        self.want = PC.oracle_frames(kw, self.pcm)
        self.pos = 0

    def counters(self, upto):
        return (self.want[upto - 1].frames_out, self.want[upto - 1].bytes_out) if upto > 0 else (0, 0)


class Slots:
    """a batch (or hx_multi handle) over `menu` and the life in each of its slots"""

    def __init__(self, b, menu, cfg, seed):
        self.b, self.menu, self.seed = b, menu, seed
        self.life = [Life(seed + i, menu[c]) for i, c in enumerate(cfg)]
        self.cfg = list(cfg)

    def started(self, idx, cfg):
        """the bookkeeping of an assign (or reset) that was just made: new lives in the listed slots"""
        for i, c in zip(idx, cfg):
            self.seed += 100
            self.life[i] = Life(self.seed + i, self.menu[c])
            self.cfg[i] = c

    def assign(self, idx, cfg, **kw):
        self.b.assign_streams(idx, cfg, **kw)
        self.started(idx, cfg)
        assert [self.b.stream_config(i) for i in range(len(self.life))] == self.cfg

    def block(self, counts, nf):
        first = self.life[0].pcm
        blk = np.full((len(self.life), nf * 1152) + first.shape[1:], np.nan, np.float32)
        for s, n in enumerate(counts):
            L = self.life[s]
            blk[s, :n * 1152] = L.pcm[L.pos * 1152:(L.pos + n) * 1152]
        return blk

    def call(self, counts, nf, tag=""):
        """one host call under counts: rows, counters and CRCs against every slot's life; advances the lives"""
        self.b.frame_counts(counts)
        bs, stats, crc = self.b.encode_host(self.block(counts, nf), stats=True, crc=True)
        assert self.b.status() == 0
        self.check(counts, nf, bs, stats, crc, tag)

    def check(self, counts, nf, bs, stats=None, crc=None, tag=""):
        for s, n in enumerate(counts):
            L = self.life[s]
            p = L.pos
            at = "%s slot %d (entry %d, count %d)" % (tag, s, self.cfg[s], n)
            assert bs[s] == b"".join(w.bs for w in L.want[p:p + n]), at + ": bitstream"
            for f in range(nf if stats is not None else 0):
                upto = p + min(f + 1, n)
                assert tuple(stats[s, f]) == L.counters(upto), at + " frame %d: frames / bytes emitted so far" % f
                e = L.counters(upto)[1] - L.counters(p)[1]
                assert int(crc[s, f]) == host_crc(bs[s][:e]), at + " frame %d: MusicCRC" % f
            L.pos = p + n


def menu_batch(menu, cfg=None, n=S, max_frames=MAXF):
    return api.Batch.menu(controls(menu), n, cfg=cfg, max_frames=max_frames)


def same_but_class(a, b):
    """two blobs that differ at most in the class index, the first word of the stream record behind the 24-byte header: it
    is the numbering of the batch the blob was saved from, and a restore replaces it with the receiving batch's"""
    return a[:24] == b[:24] and a[28:] == b[28:]


def test_assign_equals_a_fresh_stream(k6_build):
    """two uneven calls, slots [4, 1] handed entries [2, 3], three more calls: the assigned slots are new streams of their
    entry from the assign on, the other four run through all five calls, and a slot that sits a call out keeps its blob.
    Entry 3 is the menu's only DC-blocker entry and no slot starts with it: the PCM staging comes from the menu"""
    b = menu_batch(MENU)
    assert b.nconfigs() == 4 and [b.stream_config(i) for i in range(S)] == [0] * S
    sl = Slots(b, MENU, [0] * S, 3000)
    for c, counts in enumerate([[3, 2, 0, 4, 3, 1], [2, 4, 1, 0, 3, 2]]):
        idle = [i for i in range(S) if counts[i] == 0]
        before = states(b, idle)
        sl.call(counts, 4, "call %d" % c)
        assert states(b, idle) == before, "a slot that sat call %d out changed" % c
    before = states(b)
    sl.assign([4, 1], [2, 3])
    after = states(b)
    # ... a new menu batch whose slots start on those entries, and slot 0 of a batch created with the entry's control alone
    # (whose class index, the first word of the stream record, is that batch's own numbering: 0)
    new = menu_batch(MENU, cfg=[0, 3, 0, 0, 2, 0])
    fresh = states(new)
    new.close()
    for i in range(S):
        assert after[i] == (fresh[i] if i in (4, 1) else before[i]), i
    for i, c in ((4, 2), (1, 3)):
        one = api.Batch(api.default_control(**MENU[c]), nstreams=1, max_frames=MAXF)
        alone = one.get_stream_state(0)
        one.close()
        assert same_but_class(after[i], alone), i
    for c, counts in enumerate([[1, 3, 2, 4, 0, 3], [4, 0, 3, 1, 4, 2], [2, 2, 2, 0, 3, 1]]):
        idle = [i for i in range(S) if counts[i] == 0]
        before = states(b, idle)
        sl.call(counts, 4, "call %d after the assign" % c)
        assert states(b, idle) == before
    for i in range(S):
        assert b.frames_bytes(i) == sl.life[i].counters(sl.life[i].pos), i
    b.close()


def s16_life(seed, kw, F):
    x = synth.stream_pcm(seed, 24, sr=kw.get("samprate", 44100), bursts=True)[9 * 1152:(9 + F) * 1152]
    return np.ascontiguousarray(x)


@pytest.mark.parametrize("counts", [False, True], ids=["uniform", "per_stream_counts"])
def test_assign_between_pipelined_submits_without_a_wait(counts, k6_build):
    """submit, assign_streams, submit on one stream with two output sets in turn, then wait: the assign is ordered behind
    the first submit (its deferred packing included) and in front of the second, and changes the listed slots' class -
    rate, bitrate mode and DC blocker; under counts some assigned slots sat the first submit out"""
    import torch
    F1, F2 = 6, 5
    idx, cfg = [5, 0, 2], [1, 3, 2]
    n1 = [0, 6, 4, 5, 6, 0] if counts else [F1] * S
    n2 = [5, 5, 3, 0, 4, 5] if counts else [F2] * S
    second = [0] * S
    for i, c in zip(idx, cfg):
        second[i] = c
    a1 = [s16_life(1500 + i, MENU[0], F1) for i in range(S)]
    a2 = [s16_life(1600 + i, MENU[second[i]], F2) for i in range(S)]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    d_pcm = [torch.from_numpy(np.stack(a1)).to(dev), torch.from_numpy(np.stack(a2)).to(dev)]
    b = menu_batch(MENU)
    stride = b.out_stride(7)
    d_out = [torch.zeros((S, stride), dtype=torch.uint8, device=dev) for _ in range(2)]
    d_nb = [torch.zeros((S,), dtype=torch.int32, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    if counts:
        b.frame_counts(n1)
    b.submit_device(d_pcm[0].data_ptr(), F1, d_out[0].data_ptr(), stride, d_nb[0].data_ptr(), st)
    b.assign_streams(idx, cfg, st)
    if counts:
        b.frame_counts(n2)
    b.submit_device(d_pcm[1].data_ptr(), F2, d_out[1].data_ptr(), stride, d_nb[1].data_ptr(), st)
    b.wait(st)
    torch.cuda.synchronize()
    assert b.status() == 0
    got = []
    for c in range(2):
        o, n = d_out[c].cpu().numpy(), d_nb[c].cpu().numpy()
        got.append([o[s, :n[s]].tobytes() for s in range(S)])
    for i in range(S):
        first = oracle_bytes(MENU[0], a1[i][:n1[i] * 1152])
        assert got[0][i] == first, i
        if i in idx:
            assert got[1][i] == oracle_bytes(MENU[second[i]], a2[i][:n2[i] * 1152]), i
        else:
            both = oracle_bytes(MENU[0], np.concatenate([a1[i][:n1[i] * 1152], a2[i][:n2[i] * 1152]]))
            assert both[:len(first)] == first and got[1][i] == both[len(first):], i
    b.close()


def test_assign_to_the_present_entry_is_reset_streams(k6_build):
    """two batches over one menu, slots on several entries, the same first call; one resets slots [5, 0, 2], the other
    assigns them the entries they run: the listed slots' blobs are the same bytes in both - a new batch's - the other
    slots keep theirs, and the next call encodes the same in both.  (Blobs of running streams are compared within a batch
    only: the ring of pending main data keeps whatever bytes lie behind its frames.)"""
    cfg = [1, 0, 2, 3, 1, 2]
    twins = [Slots(menu_batch(MENU, cfg), MENU, cfg, 3300) for _ in range(2)]
    for t in twins:
        t.call([3, 4, 2, 4, 1, 3], 4, "first call")
    before = [states(t.b) for t in twins]
    idx = [5, 0, 2]
    twins[0].b.reset_streams(idx)
    twins[0].started(idx, [cfg[i] for i in idx])
    twins[1].assign(idx, [cfg[i] for i in idx])
    after = [states(t.b) for t in twins]
    new = menu_batch(MENU, cfg)
    fresh = states(new)
    new.close()
    for i in range(S):
        for k in range(2):
            assert after[k][i] == (fresh[i] if i in idx else before[k][i]), (k, i)
            assert before[k][i] != fresh[i], (k, i)         # (the first call left something to reset)
    for t in twins:
        t.call([2, 0, 3, 1, 4, 2], 4, "second call")
    for t in twins:
        t.b.close()


OTHER = {
    "mpeg2": [dict(bitrate=32, samprate=22050), dict(bitrate=32, samprate=16000), dict(bitrate=24, samprate=24000)],
    "first_generation_dual_channel": [dict(bitrate=64, mode=2), dict(bitrate=48, mode=2)],
    "mono": [dict(bitrate=64, mode=3), dict(bitrate=48, mode=3, samprate=48000)],
}


@pytest.mark.one_k6_build
@pytest.mark.parametrize("name", list(OTHER))
def test_other_kinds_of_batch(name):
    """an MPEG-2 menu (two frames per block, three rates), a first-generation-allocator menu and a mono menu: slots move
    through the menu's entries, last and first slot included"""
    menu = OTHER[name]
    if "first_generation" in name:
        skip_unless_host_libm_is_the_restated_one()
    n = 3
    b = menu_batch(menu, n=n, max_frames=4)
    sl = Slots(b, menu, [0] * n, 3500)
    sl.call([3, 1, 4], 4, "first call")
    sl.assign([2, 0], [len(menu) - 1, 1])
    sl.call([2, 3, 4], 4, "second call")
    sl.assign([1], [1])
    sl.call([4, 2, 0], 4, "third call")
    sl.assign([2], [0])
    sl.call([1, 1, 3], 3, "fourth call")
    b.close()


def converting_menu():
    """s16 44.1 -> 44.1 kHz (a copy), s24 48 -> 44.1 kHz (two stages, carried samples: the largest window), f32 44.1 -> 32 kHz
    and s16 44.1 -> 32 kHz (two stages too), all stereo"""
    return [(44100, 16, 0, 44100), (48000, 24, 0, 44100), (44100, 32, 1, 32000), (44100, 16, 0, 32000)]


def src_stream(entry, seed):
    rate, bits, is_float, target = converting_menu()[entry]
    return Stream(rate, bits, is_float, mpeg_select=target, seed=seed, seconds=1.0)


def src_expected(s, nframes):
    return s.reference(nframes) if O.ref() is not None else s.per_frame(nframes)


@pytest.mark.one_k6_build
def test_converting_batch():
    """slots that start on the menu's first entry only take streams of the others: a copy's slot and a two-stage plan's slot
    take two-stage plans (another one: the previous occupant's carried samples are in place and must not be read).  The
    schedule answers as on a new batch, in_used restarts, the bytes are the reference's, and the first call's converted PCM
    is the reference converter's"""
    A = api
    entries = [src_stream(k, 70 + k) for k in range(4)]
    b = A.SrcBatch.menu([s.ec for s in entries], [s.src for s in entries], S, max_frames=MAXF)
    assert b.nconfigs() == 4

    def schedule(bb, i):
        nb, rd = bb.schedule(i, 5)
        return nb.tolist(), rd
    new = []
    for k in range(4):
        one = A.SrcBatch([entries[k].ec], [entries[k].src], max_frames=MAXF)
        new.append(schedule(one, 0))
        assert one.in_stride(MAXF) <= b.in_stride(MAXF)
        one.close()
    occ = [src_stream(0, 80 + i) for i in range(S)]
    done, pos = [0] * S, [0] * S
    outs = [b""] * S

    def calls(frames, taps=False):
        nonlocal pos
        o, pos, pcm = run(b, occ, frames, pos=pos, taps=taps)
        for i in range(S):
            outs[i] += o[i]
            done[i] += sum(frames)
        return pcm

    def assign(idx, cfg):
        b.assign_streams(idx, cfg)
        for i, c in zip(idx, cfg):
            occ[i] = src_stream(c, 90 + 7 * i + c)
            outs[i], done[i], pos[i] = b"", 0, 0
            assert b.stream_config(i) == c and schedule(b, i) == new[c], (i, c)

    def check(tag):
        for i in range(S):
            want, used = src_expected(occ[i], done[i])
            assert outs[i] == want and pos[i] == used, "%s: slot %d" % (tag, i)

    calls([3, 4])
    check("first entry")
    assign([1, 2], [1, 3])                      # a copy's slots take two-stage plans
    pcm = calls([4], taps=True)
    if O.ref() is not None:
        for i in (1, 2):
            assert np.array_equal(pcm[0][i], ref_converted(occ[i], converting_menu()[b.stream_config(i)][3], 4)), i
    calls([2, 5])
    check("after the first assign")
    assert schedule(b, 1) != new[1]
    assign([1, 4, 2], [2, 1, 1])                # two-stage -> other two-stage (both ways), a copy -> two-stage
    pcm = calls([5], taps=True)
    if O.ref() is not None:
        for i in (1, 4, 2):
            assert np.array_equal(pcm[0][i], ref_converted(occ[i], converting_menu()[b.stream_config(i)][3], 5)), i
    calls([3])
    check("after the second assign")
    assert b.status() == 0
    b.close()


KWX = MENU[1]


@pytest.mark.one_k6_build
def test_blobs_need_the_assign_first():
    """streams saved from a batch of control X continue in slots of a menu batch after assign-to-X and restore, host and
    device form.  Without the assign the restore is refused (host) or skipped with status bit 32 (device), and the slot
    goes on as before"""
    import torch
    A = api
    F1, F2 = 5, 4
    src = A.Batch(A.default_control(**KWX), nstreams=2, max_frames=F1)
    moved = [Life(3700 + i, KWX) for i in range(2)]
    bs = src.encode_host(np.stack([L.pcm[:F1 * 1152] for L in moved]))
    for i, L in enumerate(moved):
        assert bs[i] == b"".join(w.bs for w in L.want[:F1])
        L.pos = F1
    saved = src.get_stream_states([0, 1])
    src.close()
    b = menu_batch(MENU)
    sl = Slots(b, MENU, [0] * S, 3800)
    sl.call([3, 2, 4, 1, 2, 3], 4, "first call")
    before = states(b)
    stride, need = b.states_stride(), len(saved[0])
    with pytest.raises(RuntimeError, match="entry 0: the stream state was saved under a different configuration"):
        b.set_stream_states([3], [saved[0]])
    up = np.zeros(stride, dtype=np.uint8)
    up[:need] = np.frombuffer(saved[1], dtype=np.uint8)
    d_up = torch.from_numpy(up).to("cuda:0")
    torch.cuda.synchronize()
    b.set_stream_states_device([5], d_up.data_ptr(), stride, None)
    assert b.status() == 32
    assert states(b) == before
    counts = [2, 0, 1, 3, 4, 2]
    b.frame_counts(counts)
    sl.check(counts, 4, b.encode_host(sl.block(counts, 4)), tag="after the refused restores")
    # assign, then restore: two calls each way
    sl.assign([3, 5], [1, 1])
    b.set_stream_states([3], [saved[0]])
    b.set_stream_states_device([5], d_up.data_ptr(), stride, None)
    sl.life[3], sl.life[5] = moved
    for got, want in zip(states(b, [3, 5]), saved):
        assert same_but_class(got, want)
    counts = [1, 2, 0, F2, 3, F2]
    b.frame_counts(counts)
    sl.check(counts, 4, b.encode_host(sl.block(counts, 4)), tag="after assign and restore")
    assert b.status() == 32         # (the bit of the skipped blob stays; nothing was added)
    b.close()


@pytest.mark.one_k6_build
def test_refusals_leave_the_batch_unchanged():
    A = api
    L = A.lib()
    cfg = [0, 1, 0, 2, 0, 0]
    b = menu_batch(MENU, cfg)
    sl = Slots(b, MENU, cfg, 3900)
    sl.call([3, 2, 4, 1, 2, 3], 4, "first call")
    small = [[1, 0, 2, 1, 0, 1], [0, 1, 1, 0, 2, 1], [2, 1, 0, 1, 1, 0]]
    made = [0]

    def unchanged(before, what):
        """after a refusal: every blob and every slot's entry as before, and a valid call matches the oracle"""
        assert states(b) == before and [b.stream_config(i) for i in range(S)] == cfg, what
        sl.call(small[made[0] % 3], 2, "valid call after the refusal of " + what)
        made[0] += 1
    for idx, c, n, word in (([1, 3], [0, 4], None, "entry 1: configuration 4 out of range"), ([1, 3], [-1, 0], None, "entry 0: configuration -1"),
                            ([1, 3, 1], [0, 0, 0], None, "entry 2: slot 1 is listed twice"), ([S], [0], None, "entry 0: slot 6 out of range"),
                            ([0, 1], [0, 0], -1, "n = -1")):
        ai, k = ints(idx)
        ac, _ = ints(c)
        before = states(b)
        assert L.hx_batch_assign_streams(b.h, ai, ac, k if n is None else n, None) == -1 and word in A.last_error(), (idx, c, A.last_error())
        unchanged(before, word)
    ai, k = ints([0, 1])
    before = states(b)
    assert L.hx_batch_assign_streams(b.h, None, ai, 2, None) == -1 and "idx" in A.last_error()
    unchanged(before, "a null idx")
    before = states(b)
    assert L.hx_batch_assign_streams(b.h, ai, None, 2, None) == -1 and "cfg" in A.last_error()
    unchanged(before, "a null cfg")
    before = states(b)
    assert L.hx_batch_assign_streams(b.h, None, None, 0, None) == 0         # n = 0: nothing to do, nothing launched
    unchanged(before, "n = 0")
    b.close()

    # at create: the message names the entry
    def refused(menu):
        arr = (A.EControl * len(menu))(*controls(menu))
        assert not L.hx_batch_create_menu(0, S, arr, len(menu), None, None, MAXF)
        return A.last_error()
    assert refused([MENU[0], MENU[1], dict(bitrate=64, mode=3)]).startswith("menu entry 2: mono and stereo")
    assert refused([MENU[0], dict(bitrate=32, samprate=22050)]).startswith("menu entry 1: MPEG-1 and MPEG-2")
    assert refused([MENU[0], MENU[2], MENU[0], dict(bitrate=64, mode=2)]).startswith("menu entry 3: intensity-stereo / dual-channel")
    assert refused([MENU[0], dict(bitrate=40, mode=2)]).startswith("menu entry 1: configuration rejected")
    assert refused([dict(bitrate=40, mode=2)]).startswith("menu entry 0: configuration rejected")
    # identical entries are allowed, and the caller's index comes back
    b = menu_batch([MENU[0], MENU[1], MENU[0]], cfg=[2, 1, 0, 2, 0, 1])
    assert b.nconfigs() == 3 and [b.stream_config(i) for i in range(S)] == [2, 1, 0, 2, 0, 1]
    b.assign_streams([0, 4], [0, 2])
    assert [b.stream_config(i) for i in range(S)] == [0, 1, 0, 2, 2, 1]
    b.close()
    # the create calls without a menu: their distinct controls in order of first appearance
    b = A.Batch(controls([MENU[1], MENU[0], MENU[1], MENU[2], MENU[0], MENU[1]]), max_frames=MAXF)
    assert b.nconfigs() == 3 and [b.stream_config(i) for i in range(S)] == [0, 1, 0, 2, 1, 0]
    b.close()


@pytest.mark.one_k6_build
def test_multi_assign_over_two_blocks():
    """five slots in two blocks (3 + 2) on device 0: an assign lists slots of both blocks; a bad entry that falls into the
    second block changes nothing in the first"""
    A = api
    n, nf = 5, 4
    m = A.Multi.menu(controls(MENU), n, max_frames=nf, devices=[0, 0])
    assert [m.shard(k)[1:] for k in range(2)] == [(0, 3), (3, 2)] and m.nconfigs() == 4
    sl = Slots(m, MENU, [0] * n, 4100)
    sl.call([4, 0, 2, 1, 3], nf, "first call")
    sl.assign([4, 1, 3], [3, 2, 1])
    sl.call([2, 4, 1, 3, 4], nf, "after the assign")

    def multi_states():
        out = []
        for k in range(2):
            h, (_, _, count) = m.batch(k), m.shard(k)
            for i in range(count):
                buf = (C.c_ubyte * int(A.lib().hx_batch_stream_state_bytes(h)))()
                assert A.lib().hx_batch_get_stream_state(h, i, buf) == 0
                out.append(bytes(buf))
        return out
    before = multi_states()
    for idx, cfg, word in (([0, 2, 4], [1, 1, 4], "entry 2: configuration 4 out of range"), ([1, 3, 5], [0, 0, 0], "entry 2: slot 5 out of range"),
                           ([2, 4, 4], [1, 1, 1], "entry 2: slot 4 is listed twice")):
        with pytest.raises(RuntimeError, match=word):
            m.assign_streams(idx, cfg)
    assert multi_states() == before and [m.stream_config(i) for i in range(n)] == sl.cfg
    sl.call([1, 2, 3, 0, 2], nf, "valid call after the refusals")
    m.close()


@pytest.mark.one_k6_build
@pytest.mark.parametrize("flags", [[], ["-A32000", "-B64"]], ids=["own_rates", "A32000_B64"])
def test_cli_batch_through_two_slots(flags, tmp_path):
    """`hmp3amd -batch -slots2` on five stereo files - 48 kHz s24, 44.1 kHz s16, 32 kHz f32, 44.1 kHz s16 and 48 kHz s16, of
    5, 40, 130, 3 and 101 frames: two slots take the five files one after the other, each handed over by an assign, and
    every file is byte for byte its single-file run's and, where it is built, the reference binary's"""
    files = []
    for i, (sr, fmt, frames) in enumerate([(48000, 24, 5), (44100, False, 40), (32000, True, 130), (44100, False, 3), (48000, False, 101)]):
        nsamp = frames * 1152 * (sr // 100 if flags else 320) // 320 - 301 * i - 7
        pcm = synth.stream_pcm(9700 + i, nsamp // 1152 + 1, sr=sr, rho=0.5, bursts=i != 1)[:nsamp]
        wav = str(tmp_path / ("in%d.wav" % i))
        write_wav(wav, pcm, sr, fmt)
        files.append(("file %d" % i, wav, str(tmp_path / ("slots%d.mp3" % i))))
    stderr, _ = batch_vs_single_vs_reference(files, flags, ["-slots2"], floor=1000)
    assert "5 files through 2 slots" in stderr
