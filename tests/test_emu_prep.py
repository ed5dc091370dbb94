"""The preparation stage of a decode -- base codes, site counts and stop positions, GC window classes, the smoothed content stairs and
their planes, the fixed-point content prefix sums, the signal records -- on the inputs made for it (helpers.prep_edge_cases).  The
device computes these arrays with kernels of its own that the emulator does not compile (decoder.hip: block scans, kChunkOffsets,
kStairs and the host's stairs for pieces with more runs than STAIR_RUNS, the staging of the bases in LDS); tests/test_gpu_prep.py
compares them with the emulator's array by array.  Here, on the CPU: every record meets the condition it was made for (asserted from
the emulator's arrays, so that a later change of the model files or of the inputs cannot quietly turn a record into a no-op), the
emulator's arrays agree with plain references that share no code with the kernels, and cells, score and path equal the oracle twin's."""
import numpy as np
import pytest

import augustus_amd as ax
from helpers import *


@pytest.fixture(autouse=True)
def _one_class_per_end_base(monkeypatch):
    """exact mode off, as in test_emu_cand.py: the first pass on its own, and the twin's restatement of the snippet cache off with it"""
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")
    monkeypatch.delenv("AUGX_BLK", raising=False)


def _decoded(cfg, cells=False):
    species, opts = PREP_CFGS[cfg]
    m = ax.Model(config_path(), species, **opts)
    recs = prep_edge_cases(m, cfg)
    res = emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states, cells=cells, prep=True)
    return m, recs, res


def _planes(i):
    npl = int(emu_prep(i, "nPlanes"))
    return npl, [int(c) for c in emu_prep(i, "planeCls")[:npl]]


def _blocks(i):
    return (emu_prep_off(i + 1) - emu_prep_off(i)) // scan_block()


@pytest.mark.parametrize("cfg", ["human", "human_utr"])
def test_prep_edge_cases_meet_their_conditions(cfg):
    m, recs, _ = _decoded(cfg)
    ix = {name: i for i, (name, _) in enumerate(recs)}
    ln = {name: len(s) for name, s in recs}
    win, limit = emu_gc_win(m.tables_ptr), stair_runs()
    R = {name: emu_prep_runs(i) for name, i in ix.items()}
    P = {name: _planes(i) for name, i in ix.items()}
    # the host settles runs_over, the device the two others; after the smoothing runs_over still has both classes
    assert R["runs_over"] > limit and 20000 <= ln["runs_over"] <= 40000 and P["runs_over"][0] == 2
    assert R["runs_at"] == limit and R["runs_at_plus1"] == limit + 1
    assert dict(recs)["runs_over"].startswith(dict(recs)["runs_at_plus1"]) and dict(recs)["runs_at_plus1"].startswith(dict(recs)["runs_at"])
    assert R["one_plane_after_smoothing"] > 1 and P["one_plane_after_smoothing"][0] == 1
    assert not emu_prep(ix["one_plane_after_smoothing"], "gcPlane").any()
    # a run of 999 positions between two runs of one class is dissolved, one of 1000 is kept (window starts = positions, shifted by win / 2)
    for name, length, planes in (("step_999", 999, 1), ("step_1000", 1000, 2)):
        raw = emu_prep(ix[name], "gcRaw")
        starts = (np.flatnonzero(raw[1:] != raw[:-1]) + 1).tolist()
        assert R[name] == 3 and len(starts) == 2 and starts[1] - starts[0] == length and raw[0] == raw[-1], name
        assert P[name][0] == planes, name
    raw = emu_prep(ix["short_run_first"], "gcRaw")
    starts = (np.flatnonzero(raw[1:] != raw[:-1]) + 1).tolist()
    assert starts[0] == 1 and len(starts) == 2 and starts[1] - starts[0] < 1000 and P["short_run_first"][0] == 1  # (run 0 is one window)
    assert ln["below_window"] == win - 1 and ln["at_window"] == win and R["below_window"] == R["at_window"] == 1
    assert ln["window_plus_1"] == win + 1 and R["window_plus_1"] == 2 and P["window_plus_1"][0] == 2           # (two windows, two classes)
    assert ln["window_plus_300"] == win + 300 and R["window_plus_300"] > 1
    assert ln["window_plus_1"] - win < 256 < ln["window_plus_300"] - win                    # (fewer / more windows than kStairs has threads)
    raw = emu_prep(ix["class_in_block_1_only"], "gcRaw")
    other = np.flatnonzero(raw != raw[0]) + 1                                               # (slots of the piece: window s is slot s + 1)
    assert len(other) > 0 and (other // 256 == 1).all() and P["class_in_block_1_only"][0] == 2 and emu_prep_off(ix["class_in_block_1_only"]) % 256 == 0
    assert [ln["tiny_%d" % n] for n in TINY_LENS] == list(TINY_LENS) == [1, 7, 255, 1014, 1015, 1016, 2039]
    assert [_blocks(ix["tiny_%d" % n]) for n in TINY_LENS] == [4, 4, 4, 4, 4, 8, 8]        # (1015 fills a chunk, 1016 opens a second)
    names = [name for name, _ in recs]
    assert [names[ix["tiny_%d" % n] + 1] for n in TINY_LENS[:4]] == ["tiny_%d" % n for n in TINY_LENS[1:5]]  # (next to each other)
    # site-dense neighbours: before the tiny pieces, right after the two pieces that leave only 9 pad slots
    assert names[ix["tiny_1"] - 1] == "sites_first" and names[ix["tiny_1015"] + 1] == "sites_after_tiny_1015"
    for name in ("tiny_1015", "blocks_64"):
        assert emu_prep_off(ix[name] + 1) - emu_prep_off(ix[name]) - 1 - ln[name] == 8, name   # (the before-first slot + 8 pad slots)
    for name in ("sites_first", "sites_after_tiny_1015", "sites_after_blocks_64", "tiny_1015", "tiny_2039"):
        c = emu_prep(ix[name], "cnt")[-1]
        assert sum(int(x) for x in c[4:10]) * 8 > ln[name], (name, c)                      # (a site every few bases)
    # every site kind on every slot of a scan block, and in the first and last 64 bases of the piece
    i = ix["sites_all_alignments"]
    terms = np.diff(emu_prep(i, "cnt")[:, 4:10].astype(np.int64), axis=0)[:ln["sites_all_alignments"]]
    slot = (emu_prep_off(i) + 1 + np.arange(len(terms))) % scan_block()
    for f in range(6):
        assert len(set(slot[terms[:, f] > 0].tolist())) == scan_block(), f
        assert terms[:64, f].any() and terms[-64:, f].any(), f
    assert P["n_window"][0] == 2 and "N" * win in dict(recs)["n_window"]
    soft = emu_prep(ix["softmasked"], "cnt")[:, 10]
    assert 0 < soft[-1] < ln["softmasked"]                                                 # (the model counts soft-masked bases)


@pytest.mark.parametrize("cfg", list(PREP_CFGS))
def test_prep_common_records_meet_their_conditions(cfg):
    m, recs, _ = _decoded(cfg)
    ix = {name: i for i, (name, _) in enumerate(recs)}
    assert set(PREP_COMMON) <= set(ix)
    # exactly 64, 68, 128 and 132 scan blocks: the last full step of kChunkOffsets, a tail of one chunk, two steps, two and a tail
    assert [_blocks(ix["blocks_%d" % k]) for k in (64, 68, 128, 132)] == [64, 68, 128, 132]
    assert [name for name, _ in recs][ix["blocks_64"] + 1] == "sites_after_blocks_64"
    npl, pcls = _planes(ix["planes_unordered"])
    assert npl == emu_n_classes(m.tables_ptr) and pcls == sorted(pcls, reverse=True) and pcls[0] > pcls[-1]   # (high GC first)
    if cfg in ("nasonia", "maize"):
        assert npl == {"nasonia": 5, "maize": 10}[cfg]
    if cfg == "maize":
        assert npl > 8 and emu_block_size(m.tables_ptr) > 0                                 # (more planes than the candidate kernel keeps in LDS)
    assert 1 < emu_prep_runs(ix["planes_unordered"]) <= stair_runs() and emu_prep_runs(ix["n_window"]) > 1


@pytest.mark.parametrize("cfg", list(PREP_CFGS))
def test_prep_arrays_against_plain_references(cfg):
    m, recs, _ = _decoded(cfg)
    soft_on = PREP_CFGS[cfg][1].get("softmasking") != "0"
    dense = cfg in ("human_utr", "maize")
    for i, (name, seq) in enumerate(recs):
        n = len(seq)
        b = np.frombuffer(seq.encode(), dtype=np.uint8)
        code = np.full(n, 4, dtype=np.uint8)
        for k, ch in enumerate("ACGT"):
            code[(b == ord(ch)) | (b == ord(ch.lower()))] = k
        got = emu_prep(i, "code")
        slots = emu_prep_off(i + 1) - emu_prep_off(i)
        assert len(got) == slots and slots % 1024 == 0 and slots >= n + 9
        # slot 0 is the before-first slot, the bases follow, the pad slots hold no base
        assert np.array_equal(got[1:n + 1], code) and got[0] == 4 and (got[n + 1:] == 4).all(), name
        cnt = emu_prep(i, "cnt").astype(np.int64)
        for k in range(4):  # prefix counts of a, c, g, t: numpy's cumsum; nothing is counted in the pad slots (they keep the total)
            want = np.concatenate([[0], np.cumsum(code == k), np.full(slots - n - 1, int((code == k).sum()))])
            assert np.array_equal(cnt[:, k], want), (name, "acgt"[k])
        low = np.cumsum((b >= ord("a")) & (b <= ord("z"))) if soft_on else np.zeros(n, dtype=np.int64)
        assert np.array_equal(cnt[:, 10], np.concatenate([[0], low, np.full(slots - n - 1, int(low[-1]))])), name
        assert (np.diff(cnt, axis=0) >= 0).all() and not cnt[0].any() and (np.diff(cnt[n:], axis=0) == 0).all(), name
        # stop positions: running maxima, begun afresh with every piece
        nsm = emu_prep(i, "nsm").astype(np.int64)
        assert not nsm[0].any() and (np.diff(nsm, axis=0) >= 0).all() and nsm.max() <= n, name
        # the class of every base: the plane of the base, through the piece's planes, against the classes the oracle twin decodes with
        npl, pcls = _planes(i)
        gc = twin_decode(m.tables_ptr, seq, m.n_states)[4]
        assert np.array_equal(np.asarray(pcls, dtype=np.int32)[emu_prep(i, "gcPlane")], gc), name
        assert int(emu_prep(i, "cls")) == pcls[0] and len(set(pcls)) == npl == len(set(gc.tolist())), name
        # what the read-back refuses: a plane the piece does not have, an array the model does not have
        with pytest.raises(ax.AugxError):
            emu_prep(i, "fx", npl)
        with pytest.raises(ax.AugxError):
            emu_prep(i, "code", 1)
        if not dense:
            with pytest.raises(ax.AugxError):
                emu_prep(i, "ufx")


@pytest.mark.parametrize("cfg", list(PREP_CFGS))
def test_prep_edge_cases_bit_identical_to_oracle(cfg):
    m, recs, res = _decoded(cfg, cells=True)
    for (name, seq), (st, lnv, path, V, cls) in zip(recs, res):
        rc, lnv2, path2, V2, gc = twin_decode(m.tables_ptr, seq, m.n_states, cells=True)
        assert st == 0 and rc == 0, name
        assert lnv == lnv2, name
        assert path == [(b, e, s) for b, e, s, t in path2], name
        assert np.array_equal(V, V2), name
