"""The preparation stage of augx_batch_decode on the GPU, array by array.  The kernels that make these arrays exist on the device only
(decoder.hip: kWindowClass / kClassFinal, kStairs and the host's stairs for pieces with more runs than STAIR_RUNS, the fused term + scan
kernels over blockTotals / blockScan, kChunkOffsets, the bases staged in LDS by SlotCodes); the emulator computes the same arrays with
plain loops.  On the inputs made for the branches of those kernels (helpers.prep_edge_cases; tests/test_emu_prep.py shows on the CPU that
each record meets its condition) every array of every piece read back through Batch.prep equals the emulator's, with no tolerance: the
stage is integer and fixed-point arithmetic, and doubles both sides compute from one source without contraction.  A failure names the
record, the array, the plane, the field and the first position that differs.  Cells, score and path are compared with the oracle twin
as in test_gpu_cand.py."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import augustus_amd as ax
import helpers
from helpers import *

DENSE = ("human_utr", "maize")


@pytest.fixture(autouse=True)
def _one_class_per_end_base(monkeypatch):
    """exact mode off, as in test_gpu_cand.py: the cache replays, which rewrite site values after the preparation stage, do not run"""
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")
    monkeypatch.setenv("AUGX_DEBUG_CELLS", "1")
    monkeypatch.delenv("AUGX_BLK", raising=False)


def _model(cfg):
    species, opts = PREP_CFGS[cfg]
    return ax.Model(config_path(), species, **opts)


_want = {}


def _twin(cfg, m, seq):
    if (cfg, seq) not in _want:
        rc, lnv, path, V, _ = twin_decode(m.tables_ptr, seq, m.n_states, cells=True)
        assert rc == 0
        _want[(cfg, seq)] = (lnv, path, V)
    return _want[(cfg, seq)]


def _check_prep(b, recs, dense, what):
    """every array of every piece of batch b against the emulator's last decode (of the same pieces in the same order)"""
    for i, (name, _) in enumerate(recs):
        planes = int(b.prep(i, "nPlanes")), int(emu_prep(i, "nPlanes"))
        assert planes[0] == planes[1], "%s: record %s (piece %d of %d), array nPlanes: %d against %d" % ((what, name, i, len(recs)) + planes)
        want = prep_arrays(emu_prep, i, dense)
        got = prep_arrays(b.prep, i, dense)
        assert [(w, pl) for w, pl, _ in got] == [(w, pl) for w, pl, _ in want], (what, name)
        for (which, pl, a), (_, _, e) in zip(got, want):
            d = prep_first_diff(a, e)
            assert d is None, "%s: record %s (piece %d of %d), array %s, plane %d: %s" % (what, name, i, len(recs), which, pl, d)


def _check_paths(b, cfg, m, recs, what):
    res = b.paths()
    for i, ((name, seq), r) in enumerate(zip(recs, res)):
        lnv, path, V = _twin(cfg, m, seq)
        assert r.status == 0 and r.ln_viterbi == lnv and r.states == path, (what, name)
        assert np.array_equal(b.cells(i), V), (what, name)


def _decode_and_check(d, cfg, m, recs, what, paths=True):
    """one batch: the emulator first (its arrays are those of its last decode), then the device, decoded twice -- the second decode of
    a batch skips the class kernels and the stairs"""
    emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states, prep=True)
    b = ax.Batch(d, [s for _, s in recs])
    for turn in ("first decode", "second decode"):
        b.decode()
        _check_prep(b, recs, cfg in DENSE, "%s, %s, %s" % (cfg, what, turn))
        if paths:
            _check_paths(b, cfg, m, recs, "%s, %s, %s" % (cfg, what, turn))
    return b


@pytest.mark.parametrize("order", ["given", "reversed"])
@pytest.mark.parametrize("cfg", list(PREP_CFGS))
def test_gpu_prep_arrays_equal_emulator(cfg, order):
    m = _model(cfg)
    d = ax.Decoder(m, 0)
    recs = prep_edge_cases(m, cfg)
    _decode_and_check(d, cfg, m, recs if order == "given" else recs[::-1], order).close()
    d.close()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("cfg", ["human", "human_utr"])
def test_gpu_prep_host_stairs_leave_the_device_settled_pieces_alone(cfg, where):
    """the piece with more runs than STAIR_RUNS is settled by the host, which downloads and uploads the per-piece tables of the whole
    batch: the pieces kStairs settled itself (two planes, one plane after smoothing, two windows) keep what it made, wherever the
    host's piece stands among them"""
    m = _model(cfg)
    d = ax.Decoder(m, 0)
    by = dict(prep_edge_cases(m, cfg))
    others = ["runs_at", "step_1000", "one_plane_after_smoothing", "window_plus_1", "planes_unordered", "runs_at_plus1", "n_window", "tiny_1015",
              "class_in_block_1_only"]
    at = {"first": 0, "middle": 4, "last": len(others)}[where]
    names = others[:at] + ["runs_over"] + others[at:]
    recs = [(n, by[n]) for n in names]
    b = _decode_and_check(d, cfg, m, recs, "host stairs " + where)
    runs = [emu_prep_runs(i) for i in range(len(recs))]
    assert {n for n, r in zip(names, runs) if r > stair_runs()} == {"runs_over", "runs_at_plus1"}   # (the host's pieces)
    assert sum(1 < r <= stair_runs() for r in runs) >= 6
    b.close()
    d.close()


def test_gpu_prep_buffers_that_came_back_from_the_pool():
    """one decoder, three batches in a row with the same piece lengths, so that each takes the buffers the one before gave back:
    one-class pieces, then pieces with several planes, then a piece whose windows disagree but whose stairs dissolve to one plane among
    one-class pieces -- its gcPlane is not written by kStairs and must be zero all the same"""
    cfg = "human"
    m = _model(cfg)
    d = ax.Decoder(m, 0)
    by = dict(prep_edge_cases(m, cfg))
    multi = [(n, by[n]) for n in ("planes_unordered", "runs_over", "step_1000", "n_window", "runs_at")]
    plain = [("plain_%d" % i, helpers._gc_dna(len(s), 0.30, 9500 + i)) for i, (_, s) in enumerate(multi)]
    third = [("one_plane_%d" % len(multi[0][1]), prep_one_plane_piece(m, len(multi[0][1])))] + plain[1:]
    for what, recs in (("one-class pieces", plain), ("several planes", multi), ("one plane after smoothing", third)):
        b = _decode_and_check(d, cfg, m, recs, what)
        planes = [int(b.prep(i, "nPlanes")) for i in range(len(recs))]
        runs = [emu_prep_runs(i) for i in range(len(recs))]
        if recs is plain:
            assert planes == [1] * len(recs) and runs == [1] * len(recs)
        elif recs is multi:
            assert planes == [2] * len(recs)
        else:
            assert planes == [1] * len(recs) and runs[0] > 1 and runs[1:] == [1] * (len(recs) - 1)
            assert not any(b.prep(i, "gcPlane").any() for i in range(len(recs)))
        b.close()  # (its buffers go back to the decoder's pool; the next batch has the same sizes)
    d.close()


def test_gpu_prep_refusals():
    """AUGX_E_ARG for a batch that was not decoded, a plane the piece does not have, an array the model does not have, a buffer that
    is too small -- and *n_bytes tells the size wanted"""
    m = _model("human")
    d = ax.Decoder(m, 0)
    by = dict(prep_edge_cases(m, "human"))
    b = ax.Batch(d, [by["tiny_255"], by["step_1000"]])
    L = ax.lib()
    nb = ctypes.c_int64(-1)
    buf = np.zeros(1 << 16, dtype=np.uint8)
    call = lambda piece, which, plane, cap: L.augx_batch_prep(d._h, b._h, piece, which, plane, buf.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(nb))
    assert call(0, 0, 0, buf.nbytes) == ax.AUGX_E_ARG and nb.value == 0   # (not decoded)
    b.decode()
    assert call(0, 0, 0, buf.nbytes) == 0 and nb.value == 1024
    assert call(0, 0, 0, 1023) == ax.AUGX_E_ARG and nb.value == 1024      # (too small: the size wanted)
    assert call(2, 0, 0, buf.nbytes) == ax.AUGX_E_ARG and call(-1, 0, 0, buf.nbytes) == ax.AUGX_E_ARG and call(0, 99, 0, buf.nbytes) == ax.AUGX_E_ARG
    assert call(0, 0, 1, buf.nbytes) == ax.AUGX_E_ARG                      # (code has no planes)
    assert int(b.prep(0, "nPlanes")) == 1 and int(b.prep(1, "nPlanes")) == 2
    assert b.prep(1, "fx", 1).shape == (8192, 20) and b.prep(1, "plsR", 1).shape == (len(by["step_1000"]), 3)
    for piece, plane in ((0, 1), (1, 2)):
        with pytest.raises(ax.AugxError) as e:
            b.prep(piece, "fx", plane)
        assert e.value.code == ax.AUGX_E_ARG
    for which in ("ufx", "ucnt"):                                          # (the trellis family has no UTR arrays)
        with pytest.raises(ax.AugxError):
            b.prep(0, which)
    b.close()
    d.close()


def test_gpu_decoder_and_batch_collected_together():
    """a decoder and a batch of it that become garbage in one reference cycle (as the traceback of a failed test holds them): the
    collector runs their __del__ in any order and clears weak references first; the batch must go before or with its decoder, never
    after it (it holds a pointer to it), and the device stays usable"""
    import gc
    m = _model("human")
    d = ax.Decoder(m, 0)
    b = ax.Batch(d, ["ACGT" * 200])
    b.decode()
    live = d._batches
    assert live == {b._h.value}
    cycle = [d, b]
    cycle.append(cycle)
    del d, b, cycle
    gc.collect()
    assert not live
    d2 = ax.Decoder(m, 0)
    assert d2.decode(["ACGT" * 200])[0].status == 0
    d2.close()
