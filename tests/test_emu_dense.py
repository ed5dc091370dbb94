"""The data paths of the dense kernels (dense.h: utrDescGroup, densePiece, denseBacktracePiece) that ordinary DNA rarely takes: UTR exon
cells with more units of candidates than there are candidate wavefronts, descriptors beyond the LDS staging, predecessors exactly at the
edge of the ring of 64 columns, the cell of the last base that is made twice, blocks with more records than threads, chain runs of the
back-trace that end on the edge of a step of 256 bases.  The emulator counts them (EmuDense): the inputs of helpers.dense_edge_cases
must take every one a fixture model can take, each assertion beside the condition on the input or the model that makes it so; the
paths no fixture model takes are asserted to stay untaken, so that the day a model reaches one this file says so.  On those inputs the
emulated kernels equal the oracle twin bit for bit, built as the product is and with 8 descriptors of a block in LDS
(build/libaugx_emu_smallwin.so), and the forward matrix is the live reference's.  (CPU-only; the same inputs run through the device
kernels in test_gpu_dense.py.)"""
import os

import numpy as np
import pytest

import augustus_amd as ax
from helpers import *

# (configuration, AUGX_BLK or None): the 71-state model at its own block size 4 and forced to 2, with two GC classes (human) and one
# (fly, UTR states by default); the 48-state model with two intergenic states and a 47-state model the trellis layout refuses, both at 8
DENSE_CFGS = [("human_utr", None), ("human_utr", "2"), ("fly_utr", None), ("human_atleastone", None), ("maize", None)]
CFGS = {**GOLDEN_CFGS, **GENEMODEL_CFGS, "maize": ("maize", {"UTR": "off", "sample": "0", "softmasking": "0"})}
BLOCK = {"human_utr": 4, "fly_utr": 4, "human_atleastone": 8, "maize": 8}
_want = {}


@pytest.fixture(autouse=True)
def _one_class_per_end_base(monkeypatch):
    """exact mode off, as in test_emu_trellis.py: the first pass on its own, and the twin's restatement of the snippet cache off with it"""
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")


def _model(monkeypatch, cfg, blk, **more):
    if blk is None:
        monkeypatch.delenv("AUGX_BLK", raising=False)
    else:
        monkeypatch.setenv("AUGX_BLK", blk)
    species, opts = CFGS[cfg]
    return ax.Model(config_path(), species, **{**opts, **more})


def _twin(m, cfg, seq, cells=True):
    """(status, score, path, cells, GC classes) of the twin, once per configuration and record (the twin does not know AUGX_BLK)"""
    key = (cfg, seq)
    if key not in _want:
        rc, lnv, path, V, gc = twin_decode(m.tables_ptr, seq, m.n_states, cells=cells)
        _want[key] = (rc, lnv, [(b, e, s) for b, e, s, t in path], V, len(set(gc.tolist())))
    return _want[key]


def _parity(m, cfg, recs, res):
    n_ok = 0
    for (name, seq), r in zip(recs, res):
        rc, lnv, path, V, _ = _twin(m, cfg, seq)
        # (two intergenic states: a record without room for a gene has no feasible path; its cells are compared all the same)
        assert rc == 0 or (cfg == "human_atleastone" and rc == ax.AUGX_E_NOPATH), name
        assert r[0] == rc, name
        if rc == 0:
            assert r[1] == lnv and r[2] == path, name
            n_ok += 1
        assert np.array_equal(r[3], V), name
    return n_ok


def _assert_reach(c, cfg, m, dims, lags, blk, n_multi, n_cut, smallwin):
    """what the records of dense_edge_cases are made to reach under configuration cfg at block size blk"""
    utr = m.n_states == 71
    unit, waves, ntw = dims["UNIT"], dims["CAND_WAVES"], dims["NTW"]
    assert (unit, ntw, dims["BT_STEP"]) == (128, 448, 256) and waves == (5 if blk == 8 else 7)
    if utr:
        # cag_dense, taa_after_gene: hundreds of sites in the window of one UTR exon end: several units of candidates per descriptor
        assert c["max_total"] > unit and c["desc_multi_unit"] > 0, c
        # ... under the human model (UTR exons of up to 2000 bases, a site every third base) more than unit * wavefronts: a candidate
        # wavefront takes two units of one descriptor.  The windows of the fly model hold fewer: it never does
        if cfg == "human_utr":
            assert c["max_total"] > unit * waves, c
        assert (c["desc_gt_waves"] > 0) == (c["max_total"] > unit * waves), c
        # totals of every residue: a last unit that leaves its second half empty, candidates that fill their units exactly
        assert c["last_half_empty"] > 0 and c["total_exact"] > 0, c
        # at most DUV = 16 UTR exon states end at a base: 16 * blk descriptors per block
        assert 0 < c["max_block_descs"] <= 16 * blk, c
        if smallwin:  # ... more than the 8 of the small build: the rest is read from HBM
            assert dims["UDCAP"] == 8 < c["max_block_descs"] and c["desc_hbm"] > 0, c
        else:         # ... never more than the product stages: unreachable there
            assert 16 * BLOCK[cfg] <= dims["UDCAP"] == 64 and c["desc_hbm"] == 0, c
        # the leading candidates of a descriptor with a middle part of at most one base, evaluated by the descriptor kernel
        assert c["pre_1"] > 0 and c["pre_2"] > 0 and c["pre_3"] > 0, c
        # candidates that are on no site list: windows that begin before the piece (prefix_*, every record's first bases), starts from
        # column 0, acceptor sites whose longass state would end after the piece
        for k in ("extra_tf", "extra_tm", "extra_fs", "extra_rt", "extra_la"):
            assert c[k] > 0, (k, c)
        assert c["mid_1"] > 0 and c["mid_0"] > 0 and c["mid_neg"] > 0, c
        assert c["tail3_right"] > 0 and c["tail3_left"] > 0, c
        # sites a few bases apart over kilobases: predecessor ends at every distance, 63 (ring) and 64 (HBM) among them
        assert c["at63_1"] > 0 and c["at64_1"] > 0, c
        # every piece with nucleotides that ends in an open utr3single cell makes it again; cut_*: with a live predecessor in the block
        assert n_cut > 0 and c["redo_cells"] >= n_cut and c["redo_live"] > 0, c
        # no UTR exon state of the fixture models has more than four ancestors: the loop from the fifth on never runs
        assert 0 < c["max_anc_utr"] <= 4, c
        # taa_after_gene: the path goes through a 3' UTR exon with more than 64 candidates; tttatt: two ancestors of equal value
        assert c["bt_utr_chunks"] > 0 and c["bt_tie_anc"] > 0, c
    else:
        assert not any(c[k] for k in DENSE_COVERAGE[:DENSE_COVERAGE.index("at63_0")] + ("at63_1", "at64_1", "redo_cells", "max_anc_utr", "bt_utr_chunks")), c
    # cag_many and the motif repeats: exon candidates whose predecessor ends 63 and 64 bases before the last base of the block
    assert c["at63_0"] > 0 and c["at64_0"] > 0, c
    # a fixed-lag state reads base j - lag, at distance lag + (blk - 1 - dj) from the block's last base
    assert (c["at63_2"] > 0) == any(63 - (blk - 1) <= l <= 63 for l in lags), (lags, c)
    assert (c["at64_2"] > 0) == any(64 - (blk - 1) <= l <= 64 for l in lags), (lags, c)
    if cfg == "maize":  # (its acceptor window of 64 bases is why the trellis layout refuses it)
        assert 64 in lags
    # cag_many: thousands of exon candidates per block; an open reverse frame has one stop per frame: few RTERMINAL records
    assert c["nonrt_gt_ntw"] > 0 and 0 < c["max_rt"] <= ntw, c
    # no state graph of the fixtures has a chain state with ANOTHER chain state of its own stage among its ancestors, or a late chain
    # state fed by a fixed-lag or early chain state: the general chainRun and stage 4 without the accumulators are run by nothing
    assert c["chain_general"] == 0 and c["lateacc_false"] == 0, c
    assert c["all_n"] == 4, c  # N_1, N_2, N_5, N_300
    assert c["trn_lds"] > 0 and (c["trn_hbm"] > 0) == (n_multi > 0), (n_multi, c)
    # back-trace: intergenic runs of kilobases (several steps of 256), runs that reach base 1 (every feasible record), blocks of more
    # than 64 records; the emulator always counts near ties (second passes)
    assert c["bt_step2"] > 0 and c["bt_run_base1"] > 0 and c["bt_rec_chunks"] > 0 and c["bt_near_pass"] > 0, c
    # two candidates of different predecessor ends whose sums are the same double: no input found that makes one
    assert c["bt_tie_eop"] == 0, c


def _run(monkeypatch, cfg, blk, lib, cells):
    m = _model(monkeypatch, cfg, blk)
    b = emu_block_size(m.tables_ptr, lib)
    assert b == int(blk or BLOCK[cfg])
    recs = dense_edge_cases()
    assert max(len(s) for _, s in recs) <= 25000
    emu_dense_coverage_reset(lib)
    res = emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states, cells=cells, lib=lib)
    c = emu_dense_coverage(lib, reset=True)
    return m, b, recs, res, c


def _reach(m, cfg, b, recs, c, lib):
    n_multi = sum(1 for _, s in recs if _twin(m, cfg, s)[4] > 1)
    if CFGS[cfg][0] == "human":
        assert n_multi >= 2  # (ac_tta, twoclass_gene)
    if cfg == "fly_utr":
        assert n_multi == 0
    _assert_reach(c, cfg, m, emu_dense_dims(b, lib), emu_dense_lags(m.tables_ptr, lib), b, n_multi,
                  sum(1 for n, _ in recs if n.startswith("cut_")), lib is not None)


@pytest.mark.parametrize("cfg,blk", DENSE_CFGS)
def test_dense_edge_cases_reach_every_path(monkeypatch, cfg, blk):
    m, b, recs, res, c = _run(monkeypatch, cfg, blk, None, False)
    print("dense %s block %d: %s" % (cfg, b, c))
    _reach(m, cfg, b, recs, c, None)


@pytest.mark.parametrize("lib", [None, SMALLWIN_EMU_LIB], ids=["product", "smallwin"])
@pytest.mark.parametrize("cfg,blk", DENSE_CFGS)
def test_dense_edge_cases_bit_identical_to_oracle(monkeypatch, cfg, blk, lib):
    m, b, recs, res, c = _run(monkeypatch, cfg, blk, lib, True)
    n_ok = _parity(m, cfg, recs, res)
    # (two intergenic states: at least the records that hold the whole gene of HS04636 have a path)
    assert n_ok == len(recs) or (cfg == "human_atleastone" and n_ok >= sum(1 for n, _ in recs if n.endswith("after_gene")) == 2)
    if lib is not None:
        _reach(m, cfg, b, recs, c, lib)


# ---- the back-trace's chain runs
@pytest.mark.parametrize("cfg,kmax", [("fly_utr", 31), ("maize", 31), ("human_utr", 27)])
def test_dense_backtrace_runs_at_the_step_edges(monkeypatch, cfg, kmax):
    """prefixes of the golden record softmask_all: ONE intergenic run of n - 1 bases each (asserted from the twin's path), of every length
    around the steps of 256 bases of denseBacktracePiece and down to one base"""
    m = _model(monkeypatch, cfg, None)
    recs = dense_backtrace_prefixes(kmax)
    step = emu_dense_dims(emu_block_size(m.tables_ptr))["BT_STEP"]
    assert {step * k + d for k in range(1, kmax + 1) for d in (-1, 0, 1, 2)} <= {len(s) for _, s in recs}
    emu_dense_coverage_reset()
    res = emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states)
    c = emu_dense_coverage(reset=True)
    for (name, seq), r in zip(recs, res):
        rc, lnv, path, _, _ = _twin(m, cfg, seq, cells=False)
        assert rc == 0 and path == ([(1, len(seq) - 1, path[0][2])] if len(seq) > 1 else []), name
        assert r[0] == 0 and r[1] == lnv and r[2] == path, name
    # the intergenic state of base 1 comes from itself in column 0: the walk from base n - 1 stops below base 1, after n bases, i.e.
    # ceil(n / step) steps of which the second and later ones are counted; every run reaches base 1
    assert c["bt_step2"] == sum((len(s) - 1) // step for _, s in recs if len(s) > 1), c
    assert c["bt_run_base1"] == sum(1 for _, s in recs if len(s) > 1) and c["all_n"] == 0, c


# ---- the forward pass (densePiece<BLK, 1>)
FWD_CFGS = [("human_utr_nosm", 0), ("fly_utr", 0), ("human_utr_nosm", 3), ("fly_utr", 3)]


def _fwd_close(F, fr):
    """identical live cells; |ln F - reference| <= 1e-9 |reference| + 5e-9.  Returns the largest difference in
    units of that bound"""
    assert np.array_equal(np.isfinite(F), np.isfinite(fr))
    both = np.isfinite(F)
    d = np.abs(F[both] - fr[both])
    bar = 1e-9 * np.abs(fr[both]) + 5e-9
    assert np.all(d <= bar)
    return float(np.max(d / bar)) if d.size else 0.0


@needs_ref
@pytest.mark.parametrize("cfg,t", FWD_CFGS)
def test_dense_forward_edge_cases_match_reference(tmp_path, monkeypatch, cfg, t):
    """every forward variable of the records of dense_edge_cases against the live reference, cold and at --temperature=3"""
    monkeypatch.delenv("AUGX_EXACT_MULTICLASS")  # (the replay of the reference's caches: two records have two classes under human)
    species, opts = CFGS[cfg]
    recs = dense_edge_cases()
    fa = str(tmp_path / "f.fa")
    write_fasta(fa, recs)
    extra = ["--%s=%s" % kv for kv in opts.items() if kv[0] != "sample"] + (["--temperature=%d" % t] if t else [])
    Fref = ref_forward(fa, species, extra)
    assert len(Fref) == len(recs)
    m = ax.Model(config_path(), species, **{**opts, "sample": "100", "temperature": str(t)})
    emu_dense_coverage_reset()
    res = emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states, forward=True)
    c = emu_dense_coverage(reset=True)
    worst = 0.0
    for (name, seq), fr, r in zip(recs, Fref, res):
        try:
            worst = max(worst, _fwd_close(r[5], fr))
        except AssertionError:
            raise AssertionError(name)
    print("dense forward %s t=%d: largest |ln F - reference| = %.3g of the bound 1e-9 |reference| + 5e-9" % (cfg, t, worst))
    assert c["desc_multi_unit"] > 0 and c["at63_1"] > 0 and c["at64_1"] > 0 and c["redo_cells"] > 0 and c["nonrt_gt_ntw"] > 0, c


@needs_ref
@pytest.mark.parametrize("cfg", ["human_utr_nosm", "fly_utr"])
def test_dense_forward_edge_cases_sampled_paths_match_reference(tmp_path, cfg):
    """5 paths sampled from the forward matrix of two of the records equal the live reference's NAMGene::getSampledPath state by state
    (one rand() stream over the records)"""
    species, opts = CFGS[cfg]
    byname = dict(dense_edge_cases())
    recs = [(k, byname[k]) for k in ("taa_after_gene", "cag_dense")]
    fa = str(tmp_path / "f.fa")
    write_fasta(fa, recs)
    gold = ref_samples(fa, species, ["--%s=%s" % kv for kv in opts.items() if kv[0] != "sample"], n=5)
    m = ax.Model(config_path(), species, **{**opts, "sample": "100"})
    res = emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states, samples=5)
    for (name, seq), r, g in zip(recs, res, gold):
        assert len(g) == 5
        for it in range(5):
            assert r[7][it] == [tuple(x) for x in g[it]], (name, it)
