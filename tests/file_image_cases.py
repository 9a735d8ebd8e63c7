"""The inputs of the file-image tests (tests/test_gpu_file_images.py runs them on the GPU; tests/test_file_images_abi.py checks
on the CPU, with the oracle alone, that they reach the edges they exist for).

The small shape is the ledger test's (tests/ledger_cases.py): 9 slots, files of 1 .. 20 calls in calls of 8 frames under
per-stream counts - here VBR, so that the byte counts and with them the places a piece starts at take every residue mod 16.
Slot NEVER is never begun, slot SITS_OUT sits call 1 out, slot RESTART gets a second file between calls 2 and 3, and slot
ONE_FRAME takes a single frame of call 0: the encoder emits nothing for it, so a fed live stream has a piece of 0 bytes."""
import os
import re

import numpy as np

from ledger_cases import DRAIN, NEVER, RESTART, SITS_OUT, SMALL_NCALLS, block, small_counts, small_pcm, small_restart_pcm  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = 0xA5              # what a file image holds before anything is written
CHUNK = int(re.search(r"#define HX_FILE_CHUNK (\d+)", open(os.path.join(ROOT, "hmp3_amd", "csrc", "hx_types.h")).read()).group(1))
ONE_FRAME = 3
RESTART_NCALLS, RESTART_AT = 6, 3
# head_bytes per slot: all different, chosen (with the oracle, tests/test_file_images_abi.py) so that the shape's 17 pieces
# start at 14 of the 16 residues mod 16; the one-frame calls of the small-pieces case reach all of them
HEADS = [0, 1, 3, 4, 5, 7, 8, 13, 11]
RESTART_HEAD = 2


def counts_of(given, ncalls, call):
    c = small_counts(given, ncalls, call)
    if call == 0:
        c[ONE_FRAME] = 1
    return c


def schedule():
    """the small shape as a list of steps: ("begin", slots, ncalls, heads) | ("restart", slot) | ("call", counts)"""
    S = len(SMALL_NCALLS)
    ncalls, given, call = list(SMALL_NCALLS), [0] * S, 0
    begun = [s for s in range(S) if s != NEVER]
    steps = [("begin", begun, [ncalls[s] for s in begun], [HEADS[s] for s in begun])]
    while True:
        if call == RESTART_AT:
            steps.append(("restart", RESTART))
            ncalls[RESTART], given[RESTART] = RESTART_NCALLS, 0
        c = counts_of(given, ncalls, call)
        if not any(c):
            return steps
        steps.append(("call", c))
        given = [g + n for g, n in zip(given, c)]
        call += 1


def rows_block(full, given, counts, nf, P, dtype):
    """the call's PCM rows [S, nf * 1152 * P]: stream s's next counts[s] frames of full[s] first in its row (a mono stream of
    a stereo-pitched batch: its samples back to back), silence behind its end"""
    blk = np.zeros((len(full), nf * 1152 * P), dtype)
    for s, n in enumerate(counts):
        part = full[s][given[s] * 1152:(given[s] + n) * 1152].reshape(-1)
        blk[s, :len(part)] = part
    return blk


def oracle_pieces(api, O):
    """the small shape through the CPU oracle and hx_ledger_update -> per call and fed open slot (slot, call, n, out_bytes,
    call_bytes, live before the call, dst residue): what k_file_append will be asked to do"""
    full = small_pcm()
    S = len(full)
    enc = [O.OracleEncoder(O.default_control()) for _ in range(S)]
    rec = [api.Ledger() for _ in range(S)]
    given, call, out = [0] * S, 0, []
    for step in schedule():
        if step[0] == "begin":
            for s, nc, h in zip(*step[1:]):
                rec[s] = api.ledger_open(nc, 1, h, 0)
        elif step[0] == "restart":
            s = step[1]
            rec[s] = api.ledger_open(RESTART_NCALLS, 1, RESTART_HEAD, 0)
            enc[s], full[s], given[s] = O.OracleEncoder(O.default_control()), small_restart_pcm(), 0
        else:
            counts = step[1]
            blk = block(full, given, counts, 8)
            for s, n in enumerate(counts):
                st, nb = np.zeros((n, 2), np.int32), 0
                for f in range(n):
                    nb += len(enc[s].encode_f32(blk[s, f * 1152:(f + 1) * 1152]))
                    st[f] = enc[s].frames_out(), enc[s].bytes_out()
                live = bool(rec[s].open and not rec[s].ended)
                api.ledger_update(rec[s], st, np.zeros(n, np.uint16), nb)
                if n and rec[s].open:
                    out.append((s, call, n, nb, rec[s].call_bytes, live, (rec[s].head_bytes + rec[s].bytes - rec[s].call_bytes) % 16))
                given[s] += n
            call += 1
    return out
