"""The evaluation pass of the candidate kernel (kernels.h: candTile, pass 2) on the inputs made for it (helpers.cand_edge_cases).  The
emulator counts the branches the pass takes: the inputs must reach every one of them, so that a later change of the kernel or of the
inputs cannot quietly turn them into no-ops.  On those inputs the emulated kernels stay bit-identical to the oracle, in the product's
configuration and in a build that flushes the slow queue at 5 entries (build/libaugx_emu_slowq.so: the flush before the queue is
full and the move of the rest to the front, on ordinary inputs).  (CPU-only; the same inputs run through the twelve kCand
instantiations on the GPU in test_gpu_cand.py.)"""
import os

import numpy as np
import pytest

import augustus_amd as ax
from helpers import *

SLOWQ_LIB = os.path.join(ROOT, "build", "libaugx_emu_slowq.so")
WAVE = 64

# (configuration, AUGX_BLK or None): the trellis family at block sizes 8 and 2, a second species, the dense family (UTR states)
CAND_CFGS = [("human", None), ("fly", None), ("human_utr", None), ("human", "2")]


@pytest.fixture(autouse=True)
def _one_class_per_end_base(monkeypatch):
    """exact mode off, as in test_emu.py: the first pass on its own, and the twin's restatement of the snippet cache off with it"""
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")


def _model(monkeypatch, cfg, blk):
    if blk is None:
        monkeypatch.delenv("AUGX_BLK", raising=False)
    else:
        monkeypatch.setenv("AUGX_BLK", blk)
    species, opts = GOLDEN_CFGS[cfg]
    return ax.Model(config_path(), species, **opts)


def _parity(m, recs, res):
    for (name, seq), (st, lnv, path, V, cls) in zip(recs, res):
        rc, lnv2, path2, V2, gc = twin_decode(m.tables_ptr, seq, m.n_states, cells=True)
        assert st == 0 and rc == 0, name
        assert lnv == lnv2, name
        assert path == [(b, e, s) for b, e, s, t in path2], name
        assert np.array_equal(V, V2), name


@pytest.mark.parametrize("cfg,blk", CAND_CFGS)
def test_cand_edge_cases_reach_every_branch(monkeypatch, cfg, blk):
    m = _model(monkeypatch, cfg, blk)
    assert emu_block_size(m.tables_ptr) == int(blk or {"human_utr": 4}.get(cfg, 8))
    recs = cand_edge_cases()
    emu_cand_coverage_reset()
    emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states)
    c = emu_cand_coverage(reset=True)
    must = ("tiles", "tiles_gt_wave", "tiles_gt_dcap", "rounds_a_gt_wave", "rounds_e_gt_wave", "rounds_a0", "rounds_e0",
            "chunks_a_cont", "chunks_e_cont", "full_flush", "full_flush_move", "tail_flush")
    assert all(c[k] > 0 for k in must), c
    # the product's threshold is a full wavefront: the short repeat pieces queue more than that in one round
    assert emu_slowq_at() == WAVE and c["max_ns"] > WAVE, c


@pytest.mark.parametrize("lib", [None, SLOWQ_LIB], ids=["product", "slowq5"])
@pytest.mark.parametrize("cfg,blk", CAND_CFGS)
def test_cand_edge_cases_bit_identical_to_oracle(monkeypatch, cfg, blk, lib):
    m = _model(monkeypatch, cfg, blk)
    recs = cand_edge_cases()
    emu_cand_coverage_reset(lib)
    res = emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states, cells=True, lib=lib)
    c = emu_cand_coverage(lib, reset=True)
    # (the batch holds a piece with two GC classes: the MULTI form of the kernel)
    assert len({int(x) for x in twin_decode(m.tables_ptr, dict(recs)["twoclass"], m.n_states)[4]}) == 2 or cfg == "fly"
    _parity(m, recs, res)
    if lib is not None:
        assert emu_slowq_at(lib) == 5
        assert c["full_flush"] > 100 and c["full_flush_move"] > 100, c


def test_cand_edge_long_segments(monkeypatch):
    """a piece cut into segments (AUGX_SEG_LEN=100000) with dense motif repeats across the cuts: the fix-ups' check windows come
    from the candidate kernel's tile minima"""
    monkeypatch.setenv("AUGX_SEG_LEN", "100000")
    m = _model(monkeypatch, "human", None)
    recs = [("long", cand_edge_long())]
    assert len(recs[0][1]) >= 250000
    _parity(m, recs, emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states, cells=True))
