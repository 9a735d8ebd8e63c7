"""Decoded PCM on the GPU (hx_batch_recon_buffer, include/hmp3_amd.h "decoded PCM") against the decoder of
tests/mp3_decode.py, which tests/test_recon_cases.py pins on the CPU, reading the bytes the same calls returned.

Accuracy limits: ISO 11172-4's full-accuracy limits at int16 scale - rms of the difference below 32768 * 2^-15 / sqrt(12) =
0.2887 and largest difference at most 2.0 - over every signal frame.  Everything else is equality of float bits.
The signal is followed by zero blocks until hx_batch_frames_bytes shows every signal frame emitted (at most 40: a case
that does not get there fails)."""
import numpy as np
import pytest

import mp3_decode as M
import recon_cases as R
from gpu_support import CallBufs, bits, cur_stream, dev, device_call, sync
from hmp3_amd import api
from oracle import oracle as O

pytestmark = pytest.mark.gpu
RMS_LIMIT, MAX_LIMIT = 32768.0 * 2.0 ** -15 / np.sqrt(12.0), 2.0
F = R.F_GPU
SENTINEL = np.float32(-12345.678)


@pytest.fixture(scope="module")
def huff():
    return O.huff_tables()


def make_batch(case, max_frames=F):
    how, kw, gens = R.GPU_CASES[case][:3]
    if how == "mixed":
        return api.Batch.mixed([api.default_control(**k) for k in kw], len(gens), cfg=R.MIXED_CFG, max_frames=max_frames)
    return api.Batch(api.default_control(**kw), nstreams=len(gens), max_frames=max_frames)


def case_rows(case, P):
    """float32 [S, F * 1152 * P]: the case's PCM rows (a mono stream of a P = 2 batch: its samples first in its row)"""
    gens = R.GPU_CASES[case][2]
    rows = np.zeros((len(gens), F * 1152 * P), np.float32)
    for s, g in enumerate(gens):
        x = g().reshape(-1)
        rows[s, :x.size] = x
    return rows


def frames_of(rows, f0, nf, P, chans):
    """frames f0 .. f0 + nf of the rows, laid out as a call's rows"""
    out = np.zeros((rows.shape[0], nf * 1152 * P), np.float32)
    for s, c in enumerate(chans):
        out[s, :nf * 1152 * c] = rows[s, f0 * 1152 * c:(f0 + nf) * 1152 * c]
    return out


class Runner:
    """a batch with a recon buffer: calls of its rows' frames, the bytes and the recon collected per stream"""

    def __init__(self, b, fill=None):
        import torch
        self.b, self.S, self.P = b, b.n, b.pcm_channels()
        self.chans = [b.stream_channels(i) for i in range(b.n)]
        self.bytes = [b""] * b.n
        self.recon = [[] for _ in range(b.n)]
        self.fill = fill
        self.torch = torch

    def buffer(self, nf):
        t = self.torch.full((self.S * nf * 1152 * self.P,), float(self.fill if self.fill is not None else 0.0), dtype=self.torch.float32, device=dev())
        return t

    def call(self, rows, nf, counts=None, recon=True, submit=False):
        """one call of nf frames; -> (CallBufs, recon tensor or None), not waited for when submit"""
        buf = self.buffer(nf) if recon else None
        self.b.recon_buffer(buf.data_ptr() if recon else None)
        if counts is not None:
            self.b.frame_counts(counts)
        o = device_call(self.b, rows, nf, CallBufs(self.b, nf), submit=submit, f32=True)
        if counts is not None:
            self.b.frame_counts(None)
        return o, buf

    def take(self, o, buf, nf, counts=None):
        """after the call is done: its bytes and recon blocks appended per stream -> the raw recon rows"""
        out = o.bitstreams()
        rec = buf.cpu().numpy().reshape(self.S, nf * 1152 * self.P) if buf is not None else None
        for s in range(self.S):
            self.bytes[s] += out[s]
            n = nf if counts is None else counts[s]
            if rec is not None:
                self.recon[s].append(rec[s, :n * 1152 * self.chans[s]].copy())
        return rec

    def run(self, rows, plan, submit=False):
        f0 = 0
        for nf in plan:
            o, buf = self.call(frames_of(rows, f0, nf, self.P, self.chans), nf, submit=False)
            sync()
            self.take(o, buf, nf)
            f0 += nf
        return self

    def drain(self, nsignal):
        """zero blocks until every stream has emitted its nsignal frames; the cap is 40 blocks"""
        fed = 0
        while min(self.b.frames_bytes(i)[0] for i in range(self.S)) < nsignal:
            assert fed < R.DRAIN_CAP, "%d zero blocks did not bring the signal's frames out" % R.DRAIN_CAP
            o, _ = self.call(np.zeros((self.S, 4 * 1152 * self.P), np.float32), 4, recon=False)
            sync()
            self.take(o, None, 4)
            fed += 4
        return self

    def stream_recon(self, s):
        return np.concatenate(self.recon[s])


def compare(runner, nsignal, huff, label, reaches=frozenset()):
    """every stream's recon against the decoder's output for its bytes, over the nsignal signal frames -> the largest rms;
    reaches: what the streams' signal frames together must show of the decoder's paths, by the parsed side information"""
    worst, seen = 0.0, set()
    for s in range(runner.S):
        y, frames = M.decode(runner.bytes[s], huff)
        c = runner.chans[s]
        assert len(frames) >= nsignal and all(f["decodable"] and f["nch"] == c for f in frames[:nsignal]), (label, s)
        seen |= R.features(frames[:nsignal])
        want = y[:nsignal * 1152].reshape(-1)
        got = runner.stream_recon(s)[:nsignal * 1152 * c].astype(np.float64)
        assert got.shape == want.shape, (label, s, got.shape, want.shape)
        d = got - want
        rms, big = float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())
        print("%s stream %d: rms %.6f, max %.6f (signal rms %.1f)" % (label, s, rms, big, float(np.sqrt(np.mean(want * want)))))
        assert rms < RMS_LIMIT and big <= MAX_LIMIT, (label, s, rms, big)
        worst = max(worst, rms)
    assert reaches <= seen, (label, "the case no longer reaches", sorted(reaches - seen))
    return worst


_base = {}


def base(case, build):
    """the case in one plain call of F frames on a batch of its own, per build of the stream walk: the reference the other
    tests compare with, computed once and left unchanged -> (per stream recon, per stream the call's bytes)"""
    if (case, build) not in _base:
        b = make_batch(case)
        r = Runner(b).run(case_rows(case, b.pcm_channels()), [F])
        assert b.status() == 0
        _base[case, build] = ([r.stream_recon(s) for s in range(r.S)], list(r.bytes))
        b.close()
    return _base[case, build]


def same_bits(got, want, where):
    a, b = bits(got), bits(want)
    assert a.shape == b.shape, where
    if not np.array_equal(a, b):
        i = int(np.flatnonzero(a != b)[0])
        raise AssertionError(where + ("index %d of %d" % (i, a.size), float(np.asarray(got).reshape(-1)[i]), float(np.asarray(want).reshape(-1)[i])))


# ---- 1. accuracy ----
@pytest.mark.parametrize("case", list(R.GPU_CASES))
def test_recon_is_the_decoders_output_for_the_bytes(case, huff, k6_build):
    b = make_batch(case)
    r = Runner(b).run(case_rows(case, b.pcm_channels()), [F]).drain(F)
    assert b.status() == 0
    compare(r, F, huff, case, R.GPU_CASES[case][3])
    if R.GPU_CASES[case][0] == "one" and R.GPU_CASES[case][1].get("mode") != 3:
        assert not r.stream_recon(r.S - 1).any(), "digital silence decodes to silence"
    b.close()


# ---- 2. split invariance ----
def test_recon_does_not_depend_on_how_the_frames_are_split_over_calls(k6_build):
    case = "vbr_48k_bursts"
    want, _ = base(case, k6_build)
    b = make_batch(case)
    r = Runner(b).run(case_rows(case, b.pcm_channels()), [5, 1, 6])
    for s in range(r.S):
        same_bits(r.stream_recon(s), want[s], (case, "5 + 1 + 6", s))
    b.close()


def test_recon_does_not_depend_on_slot_or_batch_size(k6_build):
    case = "cbr128_joint_rho"
    kw, gens = R.GPU_CASES[case][1], R.GPU_CASES[case][2]
    want, _ = base(case, k6_build)
    one = api.Batch(api.default_control(**kw), nstreams=1, max_frames=F)
    r1 = Runner(one).run(gens[1]().reshape(1, -1), [F])
    same_bits(r1.stream_recon(0), want[1], ("slot 0 of a batch of 1",))
    one.close()
    five = api.Batch(api.default_control(**kw), nstreams=5, max_frames=F)
    rows = np.stack([gens[k]().reshape(-1) for k in (0, 2, 1, 3, 0)])
    r5 = Runner(five).run(rows, [F])
    same_bits(r5.stream_recon(2), want[1], ("slot 2 of a batch of 5",))
    five.close()


@pytest.mark.one_k6_build
def test_recon_is_the_same_on_both_builds_of_the_stream_walk(monkeypatch):
    case = "vbr_48k_bursts"
    got = {}
    for build in ("fat", "slim"):
        monkeypatch.setenv("HMP3AMD_K6", build)
        b = make_batch(case)
        assert b.k6_variant() == (build == "slim")
        b.close()
        got[build] = base(case, build)[0]
    for s in range(len(got["fat"])):
        same_bits(got["slim"][s], got["fat"][s], ("fat against slim", s))


# ---- 3. per-stream frame counts ----
def test_blocks_behind_a_streams_count_are_not_touched_and_a_skipped_call_changes_nothing(k6_build):
    case = "cbr128_joint_rho"
    want, _ = base(case, k6_build)
    b = make_batch(case)
    r = Runner(b, fill=SENTINEL)
    rows = case_rows(case, r.P)
    h = F // 2
    counts = [h, 0, 2, h]
    # call 1: streams 0 and 3 take frames 0 .. h, stream 2 frames 0 .. 2, stream 1 sits it out
    o, buf = r.call(frames_of(rows, 0, h, r.P, r.chans), h, counts=counts)
    sync()
    rec = r.take(o, buf, h, counts).reshape(r.S, h, 1152 * r.P)
    for s, n in enumerate(counts):
        assert (rec[s, n:] == SENTINEL).all(), ("blocks >= n were written", s)
        assert not (rec[s, :n] == SENTINEL).any(), ("a block < n was left out", s)
    # call 2: every stream goes on from where it stands - stream 1 from frame 0, as in an uninterrupted run
    at = [h, 0, 2, h]
    nxt = np.zeros((r.S, h * 1152 * r.P), np.float32)
    for s in range(r.S):
        nxt[s] = rows[s, at[s] * 1152 * r.P:(at[s] + h) * 1152 * r.P]
    o, buf = r.call(nxt, h)
    sync()
    r.take(o, buf, h)
    for s in range(r.S):
        same_bits(r.stream_recon(s), want[s][:(at[s] + h) * 1152 * r.P], ("counts", s))
    b.close()


# ---- 4. reset ----
def test_a_reset_slot_starts_from_zero_state_and_its_neighbours_go_on(k6_build):
    case = "cbr128_joint_rho"
    want, _ = base(case, k6_build)
    b = make_batch(case)
    r = Runner(b)
    rows = case_rows(case, r.P)
    h = F // 2
    r.run(rows, [h])
    b.reset_streams([1], stream=cur_stream())
    nxt = frames_of(rows, h, h, r.P, r.chans)
    nxt[1] = frames_of(rows, 0, h, r.P, r.chans)[1]        # the reset slot's new stream: the same signal from its start
    o, buf = r.call(nxt, h)
    sync()
    rec = r.take(o, buf, h)
    same_bits(rec[1], want[1][:h * 1152 * r.P], ("the reset slot against a new batch's first frames",))
    for s in (0, 2, 3):
        same_bits(r.stream_recon(s), want[s], ("a neighbour of the reset slot", s))
    b.close()


def test_a_restored_stream_starts_from_zero_recon_state_whatever_the_slot_ran(k6_build):
    """the recon state is not in the checkpoint blob: a blob restored into a slot that ran another stream with recon on
    gives, by float bits, what the same blob gives in a slot of a batch that never ran anything"""
    case = "cbr128_joint_rho"
    h = F // 2
    a = make_batch(case)
    ra = Runner(a)
    rows = case_rows(case, ra.P)
    ra.run(rows, [h])
    blob = a.get_stream_states([1])
    nxt = frames_of(rows, h, h, ra.P, ra.chans)
    nxt[0] = nxt[1]                                         # slot 0 goes on with stream 1's signal, from stream 1's blob
    a.set_stream_states([0], blob)
    o, buf = ra.call(nxt, h)
    sync()
    used = ra.take(o, buf, h)[0].copy()
    assert a.status() == 0
    a.close()
    b = make_batch(case)
    rb = Runner(b)
    rb.b.recon_buffer(rb.buffer(h).data_ptr())              # (the state exists, and has carried nothing)
    b.set_stream_states([0], blob)
    o, buf = rb.call(nxt, h)
    sync()
    fresh = rb.take(o, buf, h)[0].copy()
    assert b.status() == 0
    b.close()
    assert fresh.any()
    same_bits(used, fresh, ("a restore into a used slot against a restore into a new batch",))
    # ... and not what the stream's own continuation gives: the transient of the first two granules is there
    want = base(case, k6_build)[0][1][h * 1152 * ra.P:]
    assert not np.array_equal(bits(fresh[:1152 * ra.P]), bits(want[:1152 * ra.P]))
    same_bits(fresh[2 * 1152 * ra.P:], want[2 * 1152 * ra.P:], ("behind the transient the restored stream is the uninterrupted one",))


# ---- 5. submits ----
def test_three_pipelined_submits_with_two_buffer_sets_equal_the_plain_calls(k6_build):
    case = "vbr_48k_bursts"
    want, want_bytes = base(case, k6_build)
    b = make_batch(case)
    r = Runner(b)
    rows = case_rows(case, r.P)
    nf = F // 3
    sets = [(CallBufs(b, nf), r.buffer(nf)) for _ in range(2)]
    got = [[] for _ in range(r.S)]
    pend = []
    for k in range(3):
        o, buf = sets[k % 2]
        if k >= 2:          # (the set comes round again: its submit's results are read first)
            b.wait(cur_stream())
            sync()
            for kk, oo, bb in pend:
                rec = bb.cpu().numpy().reshape(r.S, -1)
                for s in range(r.S):
                    got[s].append((kk, rec[s].copy(), oo.bitstreams()[s]))
            pend = []
        b.recon_buffer(buf.data_ptr())
        device_call(b, frames_of(rows, k * nf, nf, r.P, r.chans), nf, o, submit=True, f32=True)
        pend.append((k, o, buf))
    b.recon_buffer(None)        # (set after the submits: theirs stay in force for them)
    b.wait(cur_stream())
    sync()
    for kk, oo, bb in pend:
        rec = bb.cpu().numpy().reshape(r.S, -1)
        for s in range(r.S):
            got[s].append((kk, rec[s].copy(), oo.bitstreams()[s]))
    assert b.status() == 0
    for s in range(r.S):
        parts = sorted(got[s], key=lambda t: t[0])
        same_bits(np.concatenate([p[1] for p in parts]), want[s], ("submits", s))
        assert b"".join(p[2] for p in parts) == want_bytes[s], ("submits: bytes", s)
    b.close()


# ---- 6. no effect on the other outputs ----
def test_rows_counters_and_crc_are_the_same_with_recon_on_and_off(k6_build):
    case = "vbr_48k_bursts"
    res = {}
    for on in (False, True):
        b = make_batch(case)
        r = Runner(b)
        rows = case_rows(case, r.P)
        buf = r.buffer(F)
        b.recon_buffer(buf.data_ptr() if on else None)
        o = CallBufs(b, F, counters=True, crc=True, packets=4096).set_on(b)
        device_call(b, rows, F, o, f32=True)
        sync()
        assert b.status() == 0
        res[on] = [a.copy() for a in o.host()] + [a.copy() for a in o.packets()[:2]]
        assert on == bool(buf.cpu().numpy().any())
        b.close()
    for a, c in zip(res[False], res[True]):
        assert np.array_equal(a, c)


# ---- 7. a converting batch ----
def test_a_converting_batch_shares_the_output(huff, k6_build):
    import torch
    from src_cases import Stream, make_batch as make_src, make_rows
    s = Stream(48000, 16, 0, mpeg_select=44100, seed=61, seconds=1.0)
    b = make_src([s], F)
    assert b.pcm_channels() == 2
    r = Runner(b)
    nf = 8
    rows = make_rows(b, [s], [0], nf, [nf])
    d_rows = torch.from_numpy(rows).to(dev())
    buf = r.buffer(nf)
    b.recon_buffer(buf.data_ptr())
    o = CallBufs(b, nf)
    used = b.encode_src_counts_device(d_rows.data_ptr(), rows.shape[1], nf, None, o.ptr, o.stride, o.nb.data_ptr(), stream=cur_stream())
    sync()
    r.take(o, buf, nf)
    b.recon_buffer(None)
    pos, fed = int(used[0]), 0
    while b.frames_bytes(0)[0] < nf:            # (the source's zero tail: the same drain, through the converter)
        assert fed < R.DRAIN_CAP
        zr = np.zeros((1, b.in_stride(4)), np.uint8)
        dz = torch.from_numpy(zr).to(dev())
        o = CallBufs(b, 4)
        b.encode_src_counts_device(dz.data_ptr(), zr.shape[1], 4, None, o.ptr, o.stride, o.nb.data_ptr(), stream=cur_stream())
        sync()
        r.take(o, None, 4)
        fed += 4
    assert b.status() == 0
    compare(r, nf, huff, "48 -> 44.1 kHz s16")
    b.close()


# ---- 8. refusals ----
@pytest.mark.one_k6_build
@pytest.mark.parametrize("kw, word", [(dict(bitrate=32, samprate=22050), "22050"), (dict(bitrate=64, mode=2), "mode 2")], ids=["mpeg2_rate", "dual_channel"])
def test_the_setter_refuses_other_kinds_and_names_the_class(kw, word):
    import torch
    b = api.Batch(api.default_control(**kw), nstreams=2, max_frames=2)
    buf = torch.zeros(2 * 2 * 1152 * 2, dtype=torch.float32, device=dev())
    assert api.lib().hx_batch_recon_buffer(b.h, buf.data_ptr()) == -1
    msg = api.last_error()
    assert "class 0" in msg and word in msg, msg
    pcm = np.stack([R.gpu_pcm(70 + i, 2, sr=kw["samprate"] if "samprate" in kw else 44100) for i in range(2)])
    assert len(b.encode_host(pcm)) == 2 and b.status() == 0, "the batch encodes normally afterwards"
    b.close()


@pytest.mark.one_k6_build
def test_the_setter_refuses_a_misaligned_pointer_and_the_batch_encodes_on():
    import torch
    b = api.Batch(api.default_control(bitrate=64), nstreams=2, max_frames=2)
    buf = torch.zeros(2 * 2 * 1152 * 2 + 4, dtype=torch.float32, device=dev())
    assert api.lib().hx_batch_recon_buffer(b.h, buf.data_ptr() + 2) == -1 and "4-byte aligned" in api.last_error()
    pcm = np.stack([R.gpu_pcm(72 + i, 2) for i in range(2)])
    got, rec = b.encode_host_recon(pcm)
    assert b.status() == 0 and rec.shape == (2, 2 * 1152 * 2) and rec.any()
    want = api.Batch(api.default_control(bitrate=64), nstreams=2, max_frames=2)
    assert want.encode_host(pcm) == got
    want.close()
    b.close()
