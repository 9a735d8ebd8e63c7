"""tools/lds_waits.py on a hand-written listing: blocks, loops, the letters of the sequence and the sibling count (CPU only,
no compiler: the reports over the real units are in profiles/)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import lds_waits

LISTING = """
\t.text
_Z6guardedPf:                           ; @_Z6guardedPf
; %bb.0:                                ; %entry
\tds_read_b32 v1, v0
\ts_waitcnt lgkmcnt(0)
\ts_cbranch_scc1 .LBB0_2
.LBB0_1:                                ; %pair0
\ts_waitcnt vmcnt(0)
\tds_read_b64 v[2:3], v0
\tds_read_b64 v[4:5], v0 offset:8
\ts_waitcnt lgkmcnt(0)
\tv_add_f32_e32 v2, v2, v3
.LBB0_2:                                ; %pair1
\ts_cbranch_scc1 .LBB0_4
; %bb.3:                                ; %pair1.body
\tds_read_b64 v[2:3], v0 offset:16
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\ts_branch .LBB0_4
.LBB0_4:                                ; %loop
                                        ; =>This Inner Loop Header: Depth=1
\tds_read_b32 v6, v0
\tds_read_b32 v7, v0 offset:4
\ts_waitcnt lgkmcnt(1)
\tds_write_b32 v0, v6
\tds_max_i32 v0, v7
\ts_waitcnt lgkmcnt(0)
\ts_cbranch_vccnz .LBB0_4
; %bb.5:                                ; %exit
\ts_swappc_b64 s[30:31], s[4:5]
\ts_endpgm
.Lfunc_end0:
\t.size\t_Z6guardedPf, .Lfunc_end0-_Z6guardedPf
"""


def test_sequences_loops_and_siblings(tmp_path):
    path = tmp_path / "unit.s"
    path.write_text(LISTING)
    funcs = lds_waits.parse(str(path))
    assert [f for f, b in funcs] == ["_Z6guardedPf"]
    blocks = funcs[0][1]
    seqs = [(b[0], b[1], b[2], b[3]) for b in blocks if b[3]]
    assert seqs == [("bb.0", None, 0, "R:b"), ("BB0_1", None, 0, "RR:"), ("BB0_2", None, 0, "b"), ("bb.3", None, 0, "R:b"),
                    ("BB0_4", "BB0_4", 1, "RR.WA:b"), ("bb.5", None, 0, "c")]
    # the entry block and the two guarded pairs are blocks of "own reads, full wait" next to each other; the loop body is not
    assert lds_waits.siblings(blocks) == 3
    assert lds_waits.siblings([b for b in blocks if b[1] == "BB0_4"]) == 0


def test_a_wait_that_does_not_name_lgkmcnt_is_not_shown():
    assert lds_waits.classify("s_waitcnt vmcnt(0)") == ""
    assert lds_waits.classify("s_waitcnt vmcnt(0) lgkmcnt(2)") == "."
    assert lds_waits.classify("ds_bpermute_b32 v1, v2, v3") == "A"
