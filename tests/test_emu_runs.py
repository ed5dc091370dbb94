"""The plan over the whole device (layout.h: planSegments, runs of segments) under the emulated kernels: three records of unequal
length are cut, by the planner's own choice for 256 workgroups, into segments of unequal length with first segments shorter than the
others; every cell, score and path equals the sequential oracle twin.  (The emulator calls trellisPiece once per segment: the loop of
a workgroup over the segments of its run exists on the device only, tests/test_gpu_runs.py.)"""
import ctypes

import numpy as np
import pytest

import augustus_amd as ax
from helpers import *

RUN_LENS = (420000, 30000, 480000)  # (the short record and the first tiles of the record after it make one run, in this order and in the reverse)


def run_records():
    import bench
    return [bench.synth_contigs(1, n, 7100 + i)[0].decode() for i, n in enumerate(RUN_LENS)]


def crossing_runs(P):
    """the runs of plan P that hold segments of more than one piece"""
    segs, r0 = P["segs"], P["run_seg0"]
    return [r for r in range(P["n_runs"]) if len({int(segs[q][0]) for q in range(r0[r], r0[r + 1])}) > 1]


@pytest.fixture(autouse=True)
def _planners_choice(monkeypatch):
    monkeypatch.delenv("AUGX_SEG_LEN", raising=False)
    monkeypatch.delenv("AUGX_SEG_CHECK_TILES", raising=False)
    monkeypatch.delenv("AUGX_BLK", raising=False)
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")  # (as in test_emu.py: the first pass on its own)


def _parity(m, seqs, res):
    for seq, (st, lnv, path, V, cls) in zip(seqs, res):
        rc, lnv2, path2, V2, _ = twin_decode(m.tables_ptr, seq, m.n_states, cells=True)
        assert st == 0 and rc == 0 and lnv == lnv2, len(seq)
        assert path == [(b, e, s) for b, e, s, t in path2], len(seq)
        assert np.array_equal(V, V2), len(seq)


def test_emulated_runs_plan_equals_twin():
    m = ax.Model(config_path(), "human")
    P = ax.plan_segments(m, RUN_LENS, 256)  # (what the emulator plans: planSegments for 256 workgroups)
    segs = P["segs"]
    length = segs[:, 3] - segs[:, 2]
    assert P["n_runs"] > 0 and crossing_runs(P)
    assert len(set(length.tolist())) > 1
    heads = [int(length[q]) for q in range(len(segs)) if segs[q][1] == 0 and (q + 1 < len(segs) and segs[q + 1][0] == segs[q][0])]
    # a first segment shorter than five check lengths -- the least of every other segment: it has no fix-up of its own
    assert heads and P["check_tiles"] + 2 <= min(heads) < 5 * P["check_tiles"], heads
    seqs = run_records()
    _parity(m, seqs, emu_decode(m.tables_ptr, seqs, m.n_states, cells=True))


def test_emulated_runs_plan_jumps_over_a_run_of_n():
    """90 kb of N in a record the planner cuts by its own choice (a short record before it; the long one begins with a segment shorter
    than the others): the segments that lie in the run of N jump (chain-only tiles, then the columns ahead in one step), the fix-ups
    that cannot converge inside it give up and are continued"""
    m = ax.Model(config_path(), "human")
    seqs = [random_dna(60000, 20), random_dna(230000, 21) + "N" * 90000 + random_dna(240000, 22)]
    P = ax.plan_segments(m, [len(s) for s in seqs], 256)
    assert P["n_runs"] > 0 and P["segs"][1][3] < 5 * P["check_tiles"] < P["segs"][2][3] - P["segs"][2][2] + 1  # (the long record begins with a short segment)
    E = ctypes.CDLL(EMU_LIB)
    E.emu_jump_tiles.restype = ctypes.c_longlong
    j0 = E.emu_jump_tiles()
    res = emu_decode(m.tables_ptr, seqs, m.n_states, cells=True)
    assert E.emu_jump_tiles() - j0 >= 90000 // 64 // 2
    _parity(m, seqs, res)
