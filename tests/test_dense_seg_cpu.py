"""Segments for the dense kernels, host side: the planner's rules for dense models, augx_model_segmentable, and the passes of
dense.h: denseTiles on the CPU emulator (build/libaugx_emu_dense_seg.so: pass 1 of every segment, the fix-ups, the continuation of a
fix-up that gave up, segFinalizePiece, the back-trace over regions of different offsets) against the oracle twin, which knows no
segments: every cell with the offsets applied, the score, the path and the near-tie count, bit for bit.

Records: dense_seg_cases.py.  The human --UTR=on model (S = 71) runs at block 4 and 2, maize (47 states, dense family) at 8; their
check length is 240 tiles, so the three-segment record has 230 337 bases."""
import os

import numpy as np
import pytest

import augustus_amd as ax
from dense_seg_cases import *

EPS = TIES_EPS["human_utr"]  # (a threshold at which paths do have near ties; the same for maize)


def _plan(m, lens, slots):
    return ax.plan_segments(m, lens, slots)


def _seg_counts(pl, n):
    return [int((pl["segs"][:, 0] == p).sum()) for p in range(n)]


def test_model_segmentable():
    assert seg_model("human").segmentable() is True
    assert seg_model("human_utr").segmentable() is True
    assert seg_model("human_exactlyone").segmentable() is False
    assert seg_model("maize").segmentable() is True


@pytest.mark.parametrize("cfg", ["human_utr", "maize"])
def test_default_plan_of_dense_models(monkeypatch, cfg):
    monkeypatch.delenv("AUGX_SEG_LEN", raising=False)
    m = seg_model(cfg)
    ck = check_tiles(m)
    min_seg = 5 * ck
    n1 = 1000000
    pl = _plan(m, [n1], 256)  # one piece alone: equal segments, none shorter than min_seg
    tiles = (n1 + 63) // 64
    k = len(pl["segs"])
    assert k == tiles // min_seg > 1 and pl["n_runs"] == 0 and pl["check_tiles"] == ck
    assert [int(x) for x in pl["segs"][:, 2]] == [tiles * i // k for i in range(k)]
    assert [int(x) for x in pl["segs"][:, 3]] == [tiles * (i + 1) // k for i in range(k)]
    assert all(int(s[3] - s[2]) >= min_seg and int(s[4]) == int(s[3]) - ck - 2 for s in pl["segs"])
    # 24 pieces on 32 slots: one segment per piece (32 // 24); on 256 slots: at most 10 each, 240 in all
    lens = [160000 * 6] * 24
    assert _seg_counts(_plan(m, lens, 32), 24) == [1] * 24
    pl = _plan(m, lens, 256)
    assert _seg_counts(pl, 24) == [min(256 // 24, (lens[0] + 63) // 64 // min_seg)] * 24 and len(pl["segs"]) <= 256
    # at least as many pieces as slots: never cut, however long the pieces
    assert _seg_counts(_plan(m, [n1] * 8, 8), 8) == [1] * 8
    assert _seg_counts(_plan(m, [n1] * 9, 8), 9) == [1] * 9
    # a piece too short for two segments stays whole
    assert _seg_counts(_plan(m, [2 * min_seg * 64 - 64], 256), 1) == [1]
    assert _seg_counts(_plan(m, [2 * min_seg * 64], 256), 1) == [2]


def test_seg_len_applies_to_dense_models(monkeypatch):
    m = seg_model("human_utr")
    monkeypatch.setenv("AUGX_SEG_LEN", str(seg_len(m)))
    n3 = three_seg_bases(m)
    assert _seg_counts(_plan(m, [n3], 256), 1) == [3] and _seg_counts(_plan(m, [n3 - 64], 256), 1) == [2]
    assert _seg_counts(_plan(m, [n3] * 4, 2), 4) == [3] * 4  # (the variable cuts whatever the number of slots)
    monkeypatch.setenv("AUGX_SEG_LEN", "0")
    assert _seg_counts(_plan(m, [1000000], 256), 1) == [1]


def test_two_intergenic_states_are_never_cut(monkeypatch):
    m = seg_model("human_exactlyone")
    monkeypatch.delenv("AUGX_SEG_LEN", raising=False)
    assert _seg_counts(_plan(m, [1000000], 256), 1) == [1]
    monkeypatch.setenv("AUGX_SEG_LEN", "80000")
    assert _seg_counts(_plan(m, [1000000], 256), 1) == [1]


def test_piece_of_n_only_is_never_cut(monkeypatch):
    """the host has the bases when it plans: the emulator entry plans as augx_batch_create does"""
    m = seg_model("maize", "8", monkeypatch)
    monkeypatch.setenv("AUGX_SEG_LEN", str(seg_len(m)))
    n3 = three_seg_bases(m)
    seqs = ["N" * n3, "N" * (n3 - 1) + "A"]
    res, plan = emu_seg_decode(m, seqs)
    assert [int((plan["segs"][:, 0] == p).sum()) for p in range(2)] == [1, 3]
    T = twin_want(m, "maize", seqs[0])
    assert res[0][0] == T.rc == 0 and res[0][1] == T.lnv and res[0][2] == twin_path(T) and np.array_equal(res[0][3], T.V)


def _check(m, cfg, seq, segments):
    res, plan = emu_seg_decode(m, [seq])
    (st, lnv, path, V, ties), = res
    T = twin_want(m, cfg, seq)
    assert len(plan["segs"]) == segments and not plan["seg_status"].any(), plan
    assert st == T.rc == 0
    assert np.array_equal(V, T.V)
    assert lnv == T.lnv and path == twin_path(T)
    assert ties == T.counts(EPS)[0]
    return plan, T


@pytest.fixture
def _eps():
    assert emu_set_near_tie_eps(EPS, SEG_EMU_LIB) == 0
    yield
    emu_set_near_tie_eps(None, SEG_EMU_LIB)


@pytest.mark.parametrize("cfg,blk", SEG_MODELS)
def test_emu_three_segments(monkeypatch, _eps, cfg, blk):
    """case 1: the model's own check length -- at least one fix-up converges in pass 2; case 2: an unreachable check length -- every
    fix-up gives up, pass 3 takes the first one to the end of the piece"""
    m = seg_model(cfg, blk, monkeypatch)
    assert emu_block_size(m.tables_ptr, SEG_EMU_LIB) == int(blk)
    monkeypatch.setenv("AUGX_SEG_LEN", str(seg_len(m)))
    seq = plain_record(m)
    plan, T = _check(m, cfg, seq, 3)
    assert converged(plan), plan
    monkeypatch.setenv("AUGX_SEG_CHECK_TILES", "100000")
    plan, _ = _check(m, cfg, seq, 3)
    last = (len(seq) + 63) // 64 - 1
    assert gave_up(plan) == [1, 2] and int(plan["seg_stop2"][1]) == last, plan
    assert [int(-2 - plan["seg_stop"][q]) for q in (1, 2)] == [int(plan["segs"][q][4]) for q in (1, 2)]  # (at tlim, not past it)


@pytest.mark.parametrize("cfg,blk", [("human_utr", "4"), ("maize", "8")])
def test_emu_run_of_n_across_a_cut(monkeypatch, _eps, cfg, blk):
    """case 3: a dead start cannot converge inside a run of N; the continuation does the rest"""
    m = seg_model(cfg, blk, monkeypatch)
    monkeypatch.setenv("AUGX_SEG_LEN", str(seg_len(m)))
    plan, _ = _check(m, cfg, nrun_record(m), 3)
    assert gave_up(plan), plan


@pytest.mark.parametrize("cfg,blk", [("human_utr", "4")])
def test_emu_gene_across_a_cut(monkeypatch, _eps, cfg, blk):
    """case 4: real DNA with a gene, the cut inside one of its exons"""
    m = seg_model(cfg, blk, monkeypatch)
    monkeypatch.setenv("AUGX_SEG_LEN", str(seg_len(m)))
    seq = gene_record(m)
    plan, T = _check(m, cfg, seq, 2)
    cut = gene_cut(m)
    assert int(plan["segs"][1][2]) * 64 == cut
    classes, _ = twin_tie_classes(m.tables_ptr, m.n_states)
    across = [(bg, en, s) for bg, en, s, _ in T.path if bg < cut <= en]
    assert len(across) == 1 and classes[across[0][2]] == 2, across  # (a variable-length state: an exon) holds the bases on both sides of the cut
