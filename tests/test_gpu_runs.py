"""Pass 1 of the trellis in runs of segments on the device (k_trellis.hip: the loop of a workgroup over the segments of its run, with
a workgroup barrier between two segments outside the role switch), which the sequential emulator never executes: the three records
of tests/test_emu_runs.py in one batch, cut by the planner's own choice, at block sizes 8 and 4, role-specialised and as the common
body that flags near ties, every batch decoded twice and in both orders; once more with an unreachable check length (every fix-up
gives up: continuations and the last pass on top of runs) and on a share of the device (a run from a piece's last segment into the
next pieces).  Every cell, the score and the path equal the oracle twin's bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import augustus_amd as ax
from helpers import *
from test_emu_runs import run_records, crossing_runs

_want = {}
_seqs = []


@pytest.fixture(autouse=True)
def _planners_choice(monkeypatch):
    monkeypatch.delenv("AUGX_SEG_LEN", raising=False)
    monkeypatch.delenv("AUGX_SEG_CHECK_TILES", raising=False)
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")  # (as in test_gpu_trellis.py: the first pass on its own)
    monkeypatch.setenv("AUGX_DEBUG_CELLS", "1")


def _records():
    if not _seqs:
        _seqs.extend(run_records())
    return list(_seqs)


def _twin(m, seq):
    """the twin's (score, path, cells) of one record (it knows neither the block size nor the plan: one decode serves every test)"""
    if seq not in _want:
        rc, lnv, path, V, _ = twin_decode(m.tables_ptr, seq, m.n_states, cells=True)
        assert rc == 0
        _want[seq] = (lnv, path, V)
    return _want[seq]


def _check_batch(m, b, seqs):
    res = b.paths()
    assert len(res) == len(seqs)
    for i, (seq, r) in enumerate(zip(seqs, res)):
        lnv, path, V = _twin(m, seq)
        assert r.status == 0, i
        assert r.ln_viterbi == lnv and r.states == path, i
        assert np.array_equal(b.cells(i), V), i


def _decode_and_check(m, seqs, ties, share=1, converge=True):
    d = ax.Decoder(m, 0)
    d.count_near_ties(ties)  # (True: batches created from now on run kTrellis<., ., true>, the common body)
    if share > 1:
        d.set_share(share)
    plans = []
    for order in (seqs, seqs[::-1]):
        b = ax.Batch(d, order)
        b.decode()
        _check_batch(m, b, order)
        b.decode()  # (the same batch again: the buffers hold what the first decode left)
        _check_batch(m, b, order)
        P = b.plan()
        segs = P["segs"]
        assert P["n_runs"] > 0 and crossing_runs(P), order  # a workgroup of pass 1 went from a segment of one piece to one of the next
        fixed = [q for q in range(len(segs)) if segs[q][1] > 0]
        if converge:
            assert any(segs[q][2] - 1 <= P["seg_stop"][q] <= segs[q][4] for q in fixed), P["seg_stop"]
        else:
            assert all(P["seg_stop"][q] <= -2 for q in fixed), P["seg_stop"]
        plans.append(P)
        b.close()
    d.close()
    return plans


@pytest.mark.parametrize("ties", [False, True], ids=["roles", "common_body"])
@pytest.mark.parametrize("blk", ["8", "4"])
def test_gpu_runs_bit_identical_to_oracle(monkeypatch, blk, ties):
    monkeypatch.setenv("AUGX_BLK", blk)
    m = ax.Model(config_path(), "human")
    _decode_and_check(m, _records(), ties)


@pytest.mark.parametrize("ties", [False, True], ids=["roles", "common_body"])
def test_gpu_runs_with_every_fixup_giving_up(monkeypatch, ties):
    monkeypatch.setenv("AUGX_SEG_CHECK_TILES", "100000")
    m = ax.Model(config_path(), "human")
    _decode_and_check(m, _records(), ties, converge=False)


def test_gpu_runs_on_a_share_of_the_device():
    """planned for 1/64 of the compute units the runs are long: one goes from the last segment of a piece, begun from a dead start,
    through the short piece into the third"""
    m = ax.Model(config_path(), "human")
    plans = _decode_and_check(m, _records(), False, share=64)
    assert any(P["segs"][P["run_seg0"][r]][1] > 0 for P in plans for r in crossing_runs(P)), [P["segs"] for P in plans]
