"""The species whose translation-initiation window is shorter than a block of the dense kernels (schistosoma, galdieria,
Micromonas_pusilla, Rhopilema_esculentum): their INITIAL candidates may start from an intergenic cell of their own block and are
therefore in the late class of the dense kernels, evaluated after the late chain states of the block like RTERMINAL (dp.h:
isLateKind, DevTables::lateInitial; layout.h: chooseDenseBlock).  On the CPU: the layout, the emulator of the device kernels against
the oracle twin bit for bit, and twin / emulator + host stage against the live reference.

galdieria at its own default (--UTR=on) stays refused, for another window than the one this is about: /Constant/tss_upwindow_size
and /UtrModel/tss_end are 0 there, so a 5' UTR exon state may be one base long (dp.h: utrMinLag)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import augustus_amd as ax
from helpers import *
from shortwin_cases import *

RUN_CFGS = ["micromonas", "rhopilema", "galdieria", "schistosoma"]
SMALLWIN = os.path.join(ROOT, "build", "libaugx_emu_smallwin.so")
_twins = {}


@pytest.fixture(autouse=True)
def _threshold_back():
    yield
    emu_set_near_tie_eps(None)


def _model(monkeypatch, cfg, blk=None, **more):
    if blk is None:
        monkeypatch.delenv("AUGX_BLK", raising=False)
    else:
        monkeypatch.setenv("AUGX_BLK", blk)
    species, opts = SHORTWIN_CFGS[cfg]
    return ax.Model(shortwin_config_path(), species, **{**opts, **more})


def _twin(m, cfg, name, seq):
    """TwinTies (cells, score, path, margins of the chain cells) of one record, once per process: the twin knows no blocks"""
    if (cfg, name) not in _twins:
        _twins[(cfg, name)] = TwinTies(m.tables_ptr, seq, m.n_states, 1)
    return _twins[(cfg, name)]


@pytest.mark.parametrize("cfg", RUN_CFGS)
def test_block_size_and_late_class(monkeypatch, cfg):
    """a block size is found (before: -1, the model was refused), the model goes to the dense kernels, the late class is on; the
    block follows from the splice-site windows, no longer from the translation-initiation window"""
    m = _model(monkeypatch, cfg)
    blk = emu_block_size(m.tables_ptr)
    assert blk in (2, 4, 8)
    assert blk == (4 if cfg == "galdieria" else 8)  # (dss_start + 2 + dss_end is 8, 9, 7 and 9)
    assert m.layout() == ("dense", blk, True)
    W, ds = WINDOWS[cfg]
    assert min(W, W + 1 - ds) < 2  # (minexonlength is 1 in all four: shorter than the smallest block)
    for b in ("2", "4"):
        m2 = _model(monkeypatch, cfg, b)
        assert emu_block_size(m2.tables_ptr) == int(b) and m2.layout() == ("dense", int(b), True)


def test_galdieria_with_utr_states_stays_refused(monkeypatch):
    m = _model(monkeypatch, "galdieria_utr")
    assert m.n_states == 71 and emu_block_size(m.tables_ptr) == -1
    with pytest.raises(ax.AugxError) as e:
        m.layout()
    assert e.value.code == ax.AUGX_E_UNSUPPORTED and "signal windows too short for the dense kernels" in str(e.value)


@pytest.mark.parametrize("cfg", sorted(GOLDEN_CFGS) + sorted(MORE_CFGS) + sorted(GENEMODEL_CFGS) + ["Vitrella_brassicaformis", "maize"])
def test_models_that_ran_before_keep_the_late_class_off(monkeypatch, cfg):
    monkeypatch.delenv("AUGX_BLK", raising=False)
    species, opts = {**GOLDEN_CFGS, **MORE_CFGS, **GENEMODEL_CFGS}.get(cfg, (cfg, {"UTR": "off"}))
    m = ax.Model(config_path(), species, **opts)
    fam, blk, late = m.layout()
    assert not late and blk == emu_block_size(m.tables_ptr)
    assert fam == ("dense" if cfg in ("Vitrella_brassicaformis", "maize") or m.n_states > 48 or cfg in GENEMODEL_CFGS else "trellis")


def _late_lines(err, kind_initial=True, offsets=None):
    out = set()
    for l in err.splitlines():
        if l.startswith("emu: late in-block:"):
            w = l.split()
            st, kind, j, eop, jb = int(w[4]), int(w[6]), int(w[8]), int(w[10]), int(w[12])
            assert jb <= eop <= j and (eop < j or kind != K_INITIAL)  # (the reference keeps an INITIAL state one base long at least)
            if (kind == K_INITIAL) == kind_initial:
                out.add((j, st))
                if offsets is not None:
                    offsets.add((j - jb, j - eop))
    return out


@pytest.mark.parametrize("which", ["product", "smallwin"])
@pytest.mark.parametrize("blk", [None, "2"])
@pytest.mark.parametrize("cfg", RUN_CFGS)
def test_emulator_equals_the_twin(monkeypatch, capfd, cfg, blk, which):
    """every cell, ln V, the path, the near-tie flag of every chain cell and the count of the piece, at the block the layout chooses
    and at 2, under the product's build and the one with the smallest windows.  The order of the stages is checked from inside
    (AUGX_EMU_CHECK_LAG reports nothing), and the short reach is really taken: INITIAL cells with a live candidate whose predecessor
    ends in their own block exist for every species, and (schistosoma, motifs_path) one of them is on the chosen path"""
    lib = None if which == "product" else SMALLWIN
    m = _model(monkeypatch, cfg, blk)
    S = m.n_states
    b = emu_block_size(m.tables_ptr, lib)
    assert b == int(blk or (4 if cfg == "galdieria" else 8))
    monkeypatch.setenv("AUGX_EMU_CHECK_LAG", "1")
    monkeypatch.setenv("AUGX_EMU_LATE_LOG", "1")
    recs = shortwin_records(cfg)
    assert all(2000 <= len(s) <= 30000 for _, s in recs)
    chain = twin_chain_states(m.tables_ptr, S)
    _, kinds = twin_tie_classes(m.tables_ptr, S)
    eps = TIES_PRODUCT_EPS
    assert emu_set_near_tie_eps(eps, lib) == 0
    cells_short, path_short, offs = 0, 0, set()
    for i, (name, seq) in enumerate(recs):
        capfd.readouterr()
        (st, lnv, path, V, _), = emu_decode(m.tables_ptr, [seq], S, cells=True, prep=True, lib=lib)
        err = capfd.readouterr().err
        assert "predecessor" not in err, err[:500]  # (the messages of AUGX_EMU_CHECK_LAG)
        T = _twin(m, cfg, name, seq)
        assert st == T.rc == 0, name
        assert lnv == T.lnv and path == [(bg, en, s) for bg, en, s, _ in T.path], name
        assert np.array_equal(V, T.V), name
        flags = chain_flags_of(emu_prep(0, "bpD", lib=lib), chain, S, dense=True)
        assert ties_first_diff(flags, T, eps) is None, (name, ties_first_diff(flags, T, eps))
        assert emu_near_ties(1, lib)[0] == T.counts(eps)[0], name
        late = _late_lines(err, offsets=offs)
        assert all(np.isfinite(T.V[j, s]) for j, s in late), name
        cells_short += len(late)
        on_path = in_block_initials(T.path, kinds, b)
        assert all((en, s) in late for _, en, s in on_path), name  # (what the path takes was a live candidate of the late class)
        path_short += len(on_path)
    print("%s block %d: %d INITIAL cells with a live predecessor in their own block, %d on a chosen path" % (cfg, b, cells_short, path_short))
    # an initial exon has three bases at least (dp.h: exNotEndPart, len > 2), its state W + 3 - dss_start, one where that is less;
    # a state of r bases that ends at offset o of its block begins in it when r <= o <= block - 1
    W, ds = WINDOWS[cfg]
    assert (cells_short > 0) == (max(1, W + 3 - ds) <= b - 1), (cells_short, b)
    assert blk is not None or cells_short > 0  # (at the block the layout chooses: every species)
    # ... and every such pair occurs: the end of an INITIAL state at every offset o of a block, with a predecessor r bases back at every
    # r from the shortest state up to o
    rmin = max(1, W + 3 - ds)
    assert offs == {(o, r) for o in range(b) for r in range(rmin, o + 1)}, sorted(offs)
    if cfg == "schistosoma" and blk is None:
        assert path_short > 0


@needs_ref
@pytest.mark.parametrize("blk", [None, "2"])
@pytest.mark.parametrize("cfg", RUN_CFGS)
def test_twin_and_emulated_forward_against_the_live_reference(monkeypatch, tmp_path, cfg, blk):
    """the twin's cells and the emulator's forward variables within 1e-9 relative of the REAL reference's (the bar of test_oracle.py), the
    same cells alive, the same path; the forward pass of the emulator at the block the layout chooses and at 2 (there is no forward
    pass in the twin: the reference is the only yardstick of the forward variables on the CPU)"""
    m = _model(monkeypatch, cfg, blk)
    S = m.n_states
    species, opts = SHORTWIN_CFGS[cfg]
    extra = ["--%s=%s" % kv for kv in opts.items()]
    recs = shortwin_records(cfg)
    fa, cells = str(tmp_path / "x.fa"), str(tmp_path / "cells.bin")
    write_fasta(fa, recs)
    res, err = ref_harness(fa, species, extra, cells_file=cells, cfg=shortwin_config_path())
    assert len(res) == len(recs), err
    Fref = ref_forward(fa, species, extra, cfg=shortwin_config_path())
    emu = emu_decode(m.tables_ptr, [s for _, s in recs], S, forward=True)
    f = open(cells, "rb")
    for (name, seq), r, fr, e in zip(recs, res, Fref, emu):
        n, S2 = struct.unpack("ii", f.read(8))
        vref = np.frombuffer(f.read(n * S2 * 8), dtype=np.float64).reshape(n, S2)
        gref = np.frombuffer(f.read(n * 4), dtype=np.int32)
        T = _twin(m, cfg, name, seq)
        assert S2 == S and np.array_equal(np.isfinite(T.V), np.isfinite(vref)), name
        both = np.isfinite(vref)
        assert np.all(np.abs(T.V[both] - vref[both]) <= 1e-9 * np.abs(vref[both]) + 5e-9), name
        assert [(b, en, t) for b, en, s, t in T.path] == r["path"] and abs(T.lnv - r["lnv"]) <= 1e-9 * abs(r["lnv"]), name
        F = e[5]
        assert np.array_equal(np.isfinite(F), np.isfinite(fr)), name
        both = np.isfinite(fr)
        assert np.all(np.abs(F[both] - fr[both]) <= 1e-9 * np.abs(fr[both]) + 5e-9), name


def _emulated_gff(m, recs):
    S = m.n_states
    ns = int(m.option("sample") or 0)
    res = emu_decode(m.tables_ptr, [s for _, s in recs], S, samples=max(ns - 1, 0)) if ns > 1 else emu_decode(m.tables_ptr, [s for _, s in recs], S)
    tys = [emu_state_type(m.tables_ptr, s) for s in range(S)]
    paths = [[(b, e, s, tys[s]) for b, e, s in r[2]] for r in res]
    return format_gff_sampled(m, recs, paths, [r[7] for r in res]) if ns > 1 else format_gff(m, recs, paths)


@pytest.mark.parametrize("cfg", RUN_CFGS)
def test_emulated_gff_equals_the_golden(monkeypatch, cfg):
    """emulator + host stage at the species' defaults (99 sampled paths with the reference's generator): the reference binary's GFF"""
    m = _model(monkeypatch, cfg)
    assert m.option("sample") == "100"
    gold = open(os.path.join(GOLDEN, "golden_shortwin_%s.gff" % cfg)).read().splitlines()
    assert _emulated_gff(m, shortwin_records(cfg)) == gold
    g = json.load(open(os.path.join(GOLDEN, "golden_shortwin_paths_%s.json" % cfg)))
    if cfg == "schistosoma":  # (the reference itself predicts such an exon)
        assert sum(r["initial_in_block"]["8"] for r in g["records"]) > 0


@needs_ref
@pytest.mark.parametrize("variant", [None, "softmasking", "complete"])
@pytest.mark.parametrize("cfg", RUN_CFGS)
def test_emulated_gff_equals_the_live_reference(monkeypatch, tmp_path, cfg, variant):
    """emulator + host stage against the reference binary run here and now: the species' defaults, --softmasking=1 on records with
    lower-case stretches, --genemodel=complete.  (--singlestrand=true and --maxDNAPieceSize go through the executable: tests/
    test_shortwin_gpu.py, against the goldens of the same binary)"""
    m = _model(monkeypatch, cfg, None, **(VARIANTS[variant] if variant else {}))
    recs = variant_records(cfg, variant)
    fa = str(tmp_path / "x.fa")
    write_fasta(fa, recs)
    env = dict(os.environ, AUGUSTUS_CONFIG_PATH=shortwin_config_path())
    ref = subprocess.run([REF_AUGUSTUS] + ref_args(cfg, variant) + [fa], capture_output=True, text=True, env=env)
    assert ref.returncode == 0, ref.stderr
    body = gff_body(ref.stdout)
    assert body == open(os.path.join(GOLDEN, "golden_shortwin_%s%s.gff" % (cfg, "_" + variant if variant else ""))).read().splitlines()
    assert _emulated_gff(m, recs) == body


# ---- --singlestrand=true: the 24-state model without shadow states.  No RTERMINAL exists there: INITIAL is the whole late class
@pytest.mark.parametrize("which", ["product", "smallwin"])
@pytest.mark.parametrize("blk", [None, "2"])
@pytest.mark.parametrize("cfg", RUN_CFGS)
def test_single_strand_emulator_equals_the_twin(monkeypatch, capfd, cfg, blk, which):
    """the single-strand model of the four species: layout, then the emulator against the twin bit for bit (cells, ln V, path) on every
    record as it is and reverse-complemented -- the two runs of --singlestrand=true --, with AUGX_EMU_CHECK_LAG silent and the
    in-block INITIAL cells counted"""
    lib = None if which == "product" else SMALLWIN
    m = _model(monkeypatch, cfg, blk, singlestrand="true")
    S = m.n_states
    assert S == 24
    b = emu_block_size(m.tables_ptr, lib)
    assert b == int(blk or (4 if cfg == "galdieria" else 8)) and m.layout() == ("dense", b, True)
    _, kinds = twin_tie_classes(m.tables_ptr, S)
    assert 8 not in kinds and K_INITIAL in kinds  # (include/augx.h: AUGX_K_RTERMINAL = 8)
    monkeypatch.setenv("AUGX_EMU_CHECK_LAG", "1")
    monkeypatch.setenv("AUGX_EMU_LATE_LOG", "1")
    recs = [r for r in shortwin_records(cfg) if r[0] != "rand20k"]
    recs = recs + revcomp_records(recs)
    cells_short, offs = 0, set()
    for name, seq in recs:
        capfd.readouterr()
        (st, lnv, path, V, _), = emu_decode(m.tables_ptr, [seq], S, cells=True, lib=lib)
        err = capfd.readouterr().err
        assert "predecessor" not in err, err[:500]
        key = (cfg + "_single", name)
        if key not in _twins:
            _twins[key] = twin_decode(m.tables_ptr, seq, S, cells=True)
        rc, tlnv, tpath, TV, _ = _twins[key]
        assert st == rc == 0 and lnv == tlnv and path == [(bg, en, s) for bg, en, s, _ in tpath], name
        assert np.array_equal(V, TV), name
        assert not _late_lines(err, kind_initial=False)  # (nothing but INITIAL is late)
        cells_short += len(_late_lines(err, offsets=offs))
    W, ds = WINDOWS[cfg]
    rmin = max(1, W + 3 - ds)
    assert offs == {(o, r) for o in range(b) for r in range(rmin, o + 1)}, sorted(offs)
    assert (cells_short > 0) == (rmin <= b - 1)


@needs_ref
@pytest.mark.parametrize("blk", [None, "2"])
@pytest.mark.parametrize("cfg", RUN_CFGS)
def test_single_strand_emulator_against_the_live_reference(monkeypatch, tmp_path, cfg, blk):
    """path and ln V of the emulator under --singlestrand=true against the REAL reference (oracle/_ref/ref_harness), records as they
    are and reverse-complemented"""
    m = _model(monkeypatch, cfg, blk, singlestrand="true")
    species, opts = SHORTWIN_CFGS[cfg]
    recs = [r for r in shortwin_records(cfg) if r[0] != "rand20k"]
    recs = recs + revcomp_records(recs)
    fa = str(tmp_path / "x.fa")
    write_fasta(fa, recs)
    res, err = ref_harness(fa, species, ["--%s=%s" % kv for kv in {**opts, "singlestrand": "true"}.items()], cfg=shortwin_config_path())
    assert len(res) == len(recs), err
    emu = emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states)
    n_genes = 0
    for (name, _), r, e in zip(recs, res, emu):
        assert e[0] == 0 and [(bg, en, emu_state_type(m.tables_ptr, st)) for bg, en, st in e[2]] == r["path"], name
        assert abs(e[1] - r["lnv"]) <= 1e-9 * abs(r["lnv"]), name
        n_genes += len(r["path"]) > 1
    assert n_genes > 0 or cfg == "micromonas"
