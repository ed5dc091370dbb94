"""The inputs made for the candidate kernel's evaluation pass (helpers.cand_edge_cases; tests/test_emu_cand.py shows that they reach
every branch of it, the flush of a full slow queue included) through the twelve kCand<BLK, MULTI, DENSE> instantiations on the GPU:
every cell, the score and the path equal the oracle twin's, on the first decode of a batch and on the second, which skips the read-back
of the candidate count."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import augustus_amd as ax
from helpers import *


@pytest.fixture(autouse=True)
def _one_class_per_end_base(monkeypatch):
    """exact mode off, as in test_gpu_parity.py: decoders are created with the first pass on its own, and the twin's restatement of the
    snippet cache is off with it"""
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")


# (configuration, AUGX_BLK): the block size the kernels take (layout.h: chooseBlockSize, chooseDenseBlock), the family.  The model with
# UTR states caps the dense kernels' block at 4 (its signal windows), so the dense family at 8 is the 48-state model with two
# intergenic states; its short pieces have no feasible path (a gene is required), their cells are compared all the same
CAND_GPU = [("human", "8"), ("human", "4"), ("human", "2"), ("human_atleastone", "8"), ("human_utr", "4"), ("human_utr", "2")]


def _check_batch(b, seqs, want):
    res = b.paths()
    assert len(res) == len(seqs)
    for i, (seq, r) in enumerate(zip(seqs, res)):
        rc, lnv, path, V = want[seq]
        assert r.status == rc, i
        if rc == 0:
            assert r.ln_viterbi == lnv and r.states == path, i
        assert np.array_equal(b.cells(i), V), i


@pytest.mark.parametrize("cfg,blk", CAND_GPU)
def test_gpu_cand_edge_cases_bit_identical_to_oracle(monkeypatch, cfg, blk):
    monkeypatch.setenv("AUGX_BLK", blk)
    monkeypatch.setenv("AUGX_DEBUG_CELLS", "1")
    species, opts = {**GOLDEN_CFGS, **GENEMODEL_CFGS}[cfg]
    m = ax.Model(config_path(), species, **opts)
    d = ax.Decoder(m, 0)
    recs = cand_edge_cases()
    want, classes = {}, {}
    for name, seq in recs:
        rc, lnv, path, V, gc = twin_decode(m.tables_ptr, seq, m.n_states, cells=True)
        assert rc == 0 or (cfg == "human_atleastone" and rc == ax.AUGX_E_NOPATH), name
        want[seq] = (rc, lnv, path, V)
        classes[name] = len(set(gc.tolist()))
    # one batch of one-class pieces (kCand<BLK, false, DENSE>), one with the two-class record in it (kCand<BLK, true, DENSE>)
    assert classes.pop("twoclass") == 2 and set(classes.values()) == {1}
    for seqs in ([s for n, s in recs if n != "twoclass"], [s for _, s in recs]):
        b = ax.Batch(d, seqs)
        b.decode()
        _check_batch(b, seqs, want)
        b.decode()  # (the same batch again: the steady state, without the read-back of the candidate count)
        _check_batch(b, seqs, want)
        b.close()
    d.close()


def test_gpu_cand_edge_long_segments(monkeypatch):
    """a piece cut into segments (AUGX_SEG_LEN=100000) with dense motif repeats across the cuts: the trellis fix-ups size their check
    window from the candidate kernel's tile minima"""
    monkeypatch.setenv("AUGX_SEG_LEN", "100000")
    monkeypatch.setenv("AUGX_DEBUG_CELLS", "1")
    m = ax.Model(config_path(), "human")
    d = ax.Decoder(m, 0)
    seqs = [cand_edge_long()] + [s for n, s in cand_edge_cases() if n.startswith("cata")]
    assert len(seqs[0]) >= 250000
    want = {}
    for seq in seqs:
        rc, lnv, path, V, _ = twin_decode(m.tables_ptr, seq, m.n_states, cells=True)
        assert rc == 0
        want[seq] = (rc, lnv, path, V)
    b = ax.Batch(d, seqs)
    b.decode()
    _check_batch(b, seqs, want)
    b.decode()
    _check_batch(b, seqs, want)
    b.close()
    d.close()
