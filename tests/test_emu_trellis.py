"""The data paths of the trellis kernel (kernels.h: trellisItems, loadTileThread, trellisPiece), of its segment bookkeeping
(segFinalizePiece) and of the forward kernel (forwardPiece) that ordinary DNA almost never takes: predecessor values that left the LDS
windows and are read back from HBM, tiles with more candidates than the LDS staging holds, blocks with more candidates than the
forward kernel has threads, thousands of candidates summed into one forward cell.  The emulator counts them (EmuTrellis): the inputs of
helpers.trellis_edge_cases must take every one, each assertion a condition on the input that is stated with it.  On those inputs the
emulated kernels equal the oracle twin bit for bit, built with the product's windows and with the smallest ones kernels.h admits
(build/libaugx_emu_smallwin.so), and the forward matrix is the live reference's.  (CPU-only; the same inputs run through the device
kernels in test_gpu_trellis.py.)"""
import os

import numpy as np
import pytest

import augustus_amd as ax
from helpers import *

WAVE = 64

# (configuration, AUGX_BLK or None): block size 8 with two species (human: two GC classes), block size 4 (the model's own choice),
# human forced to block size 2
TRELLIS_CFGS = [("human", None), ("fly", None), ("caenorhabditis", None), ("human", "2")]
CFGS = {**GOLDEN_CFGS, "caenorhabditis": ("caenorhabditis", {"UTR": "off", "sample": "0", "softmasking": "0"})}
LISTS = range(4)


@pytest.fixture(autouse=True)
def _one_class_per_end_base(monkeypatch):
    """exact mode off, as in test_emu.py: the first pass on its own, and the twin's restatement of the snippet cache off with it"""
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")


def _model(monkeypatch, cfg, blk, **more):
    if blk is None:
        monkeypatch.delenv("AUGX_BLK", raising=False)
    else:
        monkeypatch.setenv("AUGX_BLK", blk)
    species, opts = CFGS[cfg]
    return ax.Model(config_path(), species, **{**opts, **more})


def _parity(m, recs, res):
    for (name, seq), (st, lnv, path, V, cls) in zip(recs, res):
        rc, lnv2, path2, V2, gc = twin_decode(m.tables_ptr, seq, m.n_states, cells=True)
        assert st == 0 and rc == 0, name
        assert lnv == lnv2, name
        assert path == [(b, e, s) for b, e, s, t in path2], name
        assert np.array_equal(V, V2), name


def _assert_item_paths(c, win, dims, two_classes):
    """what the records of trellis_edge_cases are made to reach, whatever the windows `win` the emulator was built with"""
    # cag_many: behind ~4000 in-frame acceptors every exon end has thousands of candidates: tiles with far more than ITEM_CAP <= 2048 of
    # them (the LDS staging is full, later chunks come from HBM, and a worker's share that begins below ITEM_CAP ends beyond it)
    assert win["ITEM_CAP"] <= 2048
    assert c["tile_full"] > 0 and c["chunk_hbm"] > 0 and c["chunk_straddle"] > 0, c
    # ag_rich / ac_rich: stop-free frames of 20 kb with a site every ~4 bases: entries thousands back, LIST_WIN <= 256
    # gt_cag / ct_tac: 600 sites two bases apart inside one intron length d: needs d > 2 * (LIST_WIN - LIST_AHEAD)
    assert dims["d"] > 2 * (win["LIST_WIN"] - win["LIST_AHEAD"])
    for sel in LISTS:
        assert c["slow_list_%d" % sel] > 0, (sel, c)
        # the entries are consecutive: where values are read back, the newest one read back and the oldest one left in LDS both occur
        assert c["pay_top_%d" % sel] > 0 and c["pay_top1_%d" % sel] > 0, (sel, c)
    # atg_ggt: igenic predecessors 0 .. 2100 bases back at every third base, blocks every 8 (4, 2): both edges of VIG_WIN <= 512
    assert win["VIG_WIN"] <= 512
    assert c["slow_vig"] > 0 and c["pay_viglo"] > 0 and c["pay_viglo1"] > 0, c
    # cag_N_cag: 3600 N = 56 tiles, more than the quiet tiles before a probe (dStateLen / 64 + 4) + JUMP_MIN = 32 + the two of the landing
    assert 3600 // WAVE > dims["dStateLen"] // WAVE + 4 + 32 + 2
    assert c["jump_restage"] > 0 and c["slow_past_jump"] > 0 and c["list_past_jump"] > 0, c
    # equalD reads its predecessor dStateLen >= 64 bases back: staged from HBM
    assert dims["dStateLen"] >= WAVE and c["longv_read"] > 0, c
    # multi_far: two GC classes under the human model
    if two_classes:
        assert c["slow_multi"] > 0, c


@pytest.mark.parametrize("cfg,blk", TRELLIS_CFGS)
def test_trellis_edge_cases_reach_every_path(monkeypatch, cfg, blk):
    m = _model(monkeypatch, cfg, blk)
    assert emu_block_size(m.tables_ptr) == int(blk or {"caenorhabditis": 4}.get(cfg, 8))
    win = emu_trellis_windows()
    assert (win["ITEM_CAP"], win["LIST_WIN"], win["VIG_WIN"]) == (2048, 256, 512)  # the product's
    recs = trellis_edge_cases()
    assert max(len(s) for _, s in recs) <= 25000
    emu_trellis_coverage_reset()
    emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states)
    c = emu_trellis_coverage(reset=True)
    two = len(set(twin_decode(m.tables_ptr, dict(recs)["multi_far"], m.n_states)[4].tolist())) == 2
    assert two == (cfg == "human")
    _assert_item_paths(c, win, emu_model_dims(m.tables_ptr), two)
    # no piece is cut, no forward pass: nothing of the segment passes or the forward kernel ran
    assert not any(c[k] for k in TRELLIS_COVERAGE if k.startswith(("fwd_", "fin_", "fix_", "p3_", "m3_", "slow_mode", "slow_dead", "flush_cmp"))), c


@pytest.mark.parametrize("lib", [None, SMALLWIN_EMU_LIB], ids=["product", "smallwin"])
@pytest.mark.parametrize("cfg,blk", TRELLIS_CFGS)
def test_trellis_edge_cases_bit_identical_to_oracle(monkeypatch, cfg, blk, lib):
    m = _model(monkeypatch, cfg, blk)
    recs = trellis_edge_cases()
    emu_trellis_coverage_reset(lib)
    res = emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states, cells=True, lib=lib)
    c = emu_trellis_coverage(lib, reset=True)
    _parity(m, recs, res)
    if lib is not None:
        win = emu_trellis_windows(lib)
        assert (win["ITEM_CAP"], win["LIST_WIN"], win["VIG_WIN"]) == (1024, 128, 128)  # (Makefile: SMALLWIN)
        _assert_item_paths(c, win, emu_model_dims(m.tables_ptr), cfg == "human")


def test_adversarial_long_frames_are_beyond_the_longest_exon(monkeypatch):
    """polyGCC / polyGGC_rev of test_emu.adversarial_cases: their reading frames of 21 kb are longer than maxexonlength, so no exon
    candidate spans them and nothing is read back from HBM for them (orf12k of trellis_edge_cases is the frame that is)"""
    from test_emu import adversarial_cases
    m = _model(monkeypatch, "human", None)
    cases = adversarial_cases()
    assert 3 * 7000 > emu_model_dims(m.tables_ptr)["max_exon_len"] > 12006
    for name, want in (("polyGCC", False), ("polyGGC_rev", False)):
        emu_trellis_coverage_reset()
        emu_decode(m.tables_ptr, [cases[name]], m.n_states)
        c = emu_trellis_coverage(reset=True)
        assert (c["slow_vig"] + sum(c["slow_list_%d" % i] for i in LISTS) > 0) == want, (name, c)
    emu_decode(m.tables_ptr, [dict(trellis_edge_cases())["orf12k"]], m.n_states)
    assert emu_trellis_coverage(reset=True)["slow_vig"] > 0
    # what the docstring of adversarial_cases does claim: aggt fills the LDS staging of its tiles, ag_rich reads acceptor values back
    emu_decode(m.tables_ptr, [cases["aggt"]], m.n_states)
    c = emu_trellis_coverage(reset=True)
    assert c["tile_full"] > 0 and c["chunk_hbm"] > 0, c
    emu_decode(m.tables_ptr, [cases["ag_rich"]], m.n_states)
    assert emu_trellis_coverage(reset=True)["slow_list_0"] > 0


SEG_ENVS = [{"AUGX_SEG_LEN": "77000"}, {"AUGX_SEG_LEN": "77000", "AUGX_SEG_CHECK_TILES": "100000"}]


@pytest.mark.parametrize("lib", [None, SMALLWIN_EMU_LIB], ids=["product", "smallwin"])
@pytest.mark.parametrize("env", SEG_ENVS, ids=["check", "nocheck"])
def test_trellis_edge_long_segments(monkeypatch, env, lib):
    """the record of helpers.trellis_edge_long cut into five segments: far predecessors across the seams in pass 1 from a dead start, in
    the fix-ups, in the continuations of pass 3 and in the last pass; with an unreachable check length every fix-up gives up, three are
    continued by the rounds of pass 3 (each to the end of the piece, over the seams of the later ones) and the fourth by the last pass"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = _model(monkeypatch, "human", None)
    recs = [("long", trellis_edge_long())]
    emu_trellis_coverage_reset(lib)
    res = emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states, cells=True, lib=lib)
    c = emu_trellis_coverage(lib, reset=True)
    _parity(m, recs, res)
    # blocks of far predecessors lie across the cuts: a dead start reads back values from before its segment (and replaces them), its
    # fix-up reads the true ones and retires what it computes comparing
    assert c["slow_dead"] > 0 and c["slow_dead_cut"] > 0 and c["slow_mode1"] > 0 and c["flush_cmp"] > 0 and c["flush_cmp_bad"] > 0, c
    if "AUGX_SEG_CHECK_TILES" in env:
        # four fix-ups, none converges; SEG_CONT_ROUNDS = 3 continuations, each to the end of the piece; one left for the last pass
        assert c["fix_converged"] == 0 and c["fix_gaveup"] == 4 and c["p3_converged"] == 0 and c["p3_to_end"] == 3 and c["m3_tiles"] > 0, c
        assert c["slow_mode2"] > 0 and c["slow_mode3"] > 0, c
        # every run reached the end: the first seam looked at ends the regions
        assert c["fin_to_end"] == 1 and c["fin_covered"] == 1 and c["fin_seam"] == 0, c
    else:
        # the fix-up that starts inside the run of N cannot converge before its limit, which lies in the run: it gives up and is continued
        # by pass 3 (nothing is left for the last pass); the others converge
        assert c["fix_gaveup"] == 1 and c["fix_converged"] == 3 and c["p3_converged"] == 1 and c["p3_to_end"] == 0 and c["m3_tiles"] == 0, c
        assert c["slow_mode2"] > 0, c
        # the continuation meets the seam of the last fix-up where it would have stopped, goes on and stops behind it: of the four
        # seams one is run over, three are recorded
        assert c["p3_at_seam"] > 0 and c["fin_overrun"] == 1 and c["fin_seam"] == 3 and c["fin_to_end"] == 0 and c["fin_covered"] == 1, c


# ---- the forward kernel
FWD_CFGS = [("human_nosm", 0), ("fly", 0), ("human_nosm", 3), ("fly", 3)]


def _fwd_close(F, fr):
    """identical live cells; |ln F - reference| <= 1e-9 |reference| + 5e-9.  Returns the largest difference in
    units of that bound's scale |reference| + 5"""
    assert np.array_equal(np.isfinite(F), np.isfinite(fr))
    both = np.isfinite(F)
    d = np.abs(F[both] - fr[both])
    assert np.all(d <= 1e-9 * np.abs(fr[both]) + 5e-9)
    return float(np.max(d / (np.abs(fr[both]) + 5))) if d.size else 0.0


@needs_ref
@pytest.mark.parametrize("cfg,t", FWD_CFGS)
def test_forward_edge_cases_match_reference(tmp_path, monkeypatch, cfg, t):
    """every forward variable of the records of trellis_edge_cases against the live reference, cold and at --temperature=3, and the
    counters of the paths they are made for"""
    monkeypatch.delenv("AUGX_EXACT_MULTICLASS")  # (the replay of the reference's snippet cache: multi_far and orf12k have two classes)
    species, opts = CFGS[cfg]
    recs = trellis_edge_cases()
    fa = str(tmp_path / "f.fa")
    write_fasta(fa, recs)
    extra = ["--%s=%s" % kv for kv in opts.items() if kv[0] != "sample"] + (["--temperature=%d" % t] if t else [])
    Fref = ref_forward(fa, species, extra)
    m = ax.Model(config_path(), species, **{**opts, "sample": "100", "temperature": str(t)})
    emu_trellis_coverage_reset()
    res = emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states, forward=True)
    c = emu_trellis_coverage(reset=True)
    worst = 0.0
    for (name, seq), fr, r in zip(recs, Fref, res):
        worst = max(worst, _fwd_close(r[5], fr))
    print("forward %s t=%d: largest |ln F - reference| / (|reference| + 5) = %.3g; counters %s" % (cfg, t, worst, {k: v for k, v in c.items() if k.startswith("fwd_")}))
    ntw = emu_trellis_windows()["NTW"]
    # cag_many: 3990 in-frame acceptors before one donor site, 8 bases of it in a block: blocks of ~30 000 candidates > NTW = 448, of which
    # the reverse-strand terminal exons (RTERMINAL) come after more than NTW others; one cell sums all 3990 (and at least that many)
    assert ntw == 448 and c["fwd_gt_ntw"] > 0 and c["fwd_nonrt_gt_ntw"] > 0, c
    assert c["fwd_max_cell"] >= 3990, c
    # a term is at most 1.0: the fullest sum is no more than the candidates of its cell, which a 64-bit sum holds for every admitted model
    assert 0 < c["fwd_max_sum"] <= c["fwd_max_cell"] + 1 <= emu_model_dims(m.tables_ptr)["fwd_cell_candidates"] <= emu_trellis_windows()["FWD_SUM_TERMS"], c
    # exons longer than the ring of 64 columns; candidates that start at base 0; a piece with one class and (human) one with two
    assert c["fwd_at_hbm"] > 0 and c["fwd_col0"] > 0 and c["fwd_trn_single"] > 0, c
    assert (c["fwd_trn_multi"] > 0) == (species == "human"), c
    assert (c["fwd_heated_over"] > 0) == (t != 0), c


@needs_ref
@pytest.mark.parametrize("cfg", ["human_nosm", "fly"])
def test_forward_edge_cases_sampled_paths_match_reference(tmp_path, cfg):
    """5 paths sampled from the forward matrix of two of the records equal the live reference's NAMGene::getSampledPath state by state
    (one rand() stream over the records)"""
    species, opts = CFGS[cfg]
    byname = dict(trellis_edge_cases())
    recs = [(k, byname[k]) for k in ("gt_cag", "cag_many")]
    fa = str(tmp_path / "f.fa")
    write_fasta(fa, recs)
    gold = ref_samples(fa, species, ["--%s=%s" % kv for kv in opts.items() if kv[0] != "sample"], n=5)
    m = ax.Model(config_path(), species, **{**opts, "sample": "100"})
    res = emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states, samples=5)
    for (name, seq), r, g in zip(recs, res, gold):
        assert len(g) == 5
        for it in range(5):
            assert r[7][it] == [tuple(x) for x in g[it]], (name, it)


ALL_SPECIES = sorted(set(v[0] for v in {**GOLDEN_CFGS, **MORE_CFGS}.values()) | {"caenorhabditis", "maize", "Vitrella_brassicaformis", "chlamy2011", "tetrahymena"})


@pytest.mark.parametrize("utr", ["off", "on"])
@pytest.mark.parametrize("species", ALL_SPECIES)
def test_forward_sum_holds_every_candidate_of_a_cell(species, utr):
    """the fixed-point sum of a forward cell (dp.h: FWD_FIX) cannot wrap: a term is at most 1.0, a cell has at most one candidate per
    ancestor (AUGX_MAX_ANC = 8) and predecessor base within the longest exon or intron, and 64 bits hold FWD_SUM_TERMS terms of 1.0.
    The bound is checked where a model is checked (layout.h: checkForwardSum, which every decoder creation passes); here for every
    species fixture, with and without UTR states (a species without UTR parameters refuses --UTR=on: nothing to check)"""
    try:
        m = ax.Model(config_path(), species, UTR=utr, softmasking="0")
    except Exception:
        assert utr == "on"
        return
    d, cap = emu_model_dims(m.tables_ptr), emu_trellis_windows()["FWD_SUM_TERMS"]
    assert cap == 1 << 18
    assert d["fwd_cell_candidates"] >= 8 * (max(d["max_exon_len"], d["d"]) + 1)
    assert d["fwd_cell_candidates"] <= cap
    assert emu_block_size(m.tables_ptr) in (8, 4, 2)  # (chooseBlockSize passed checkForwardSum)
