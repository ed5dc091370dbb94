"""The species whose translation-initiation window is shorter than a block of the dense kernels, on the device (see
tests/test_shortwin_cpu.py): the decoder is created (before: AUGX_E_UNSUPPORTED), kDense with the INITIAL candidates in the late
class against the oracle twin and the emulator, and the executable against the goldens of the reference binary."""
import os
import subprocess

import numpy as np
import pytest

import augustus_amd as ax
from helpers import *
from shortwin_cases import *

pytestmark = pytest.mark.gpu
RUN_CFGS = ["micromonas", "rhopilema", "galdieria", "schistosoma"]
EXE = os.path.join(ROOT, "augustus_amd", "bin", "augustus")


def _model(monkeypatch, cfg, blk=None):
    if blk is None:
        monkeypatch.delenv("AUGX_BLK", raising=False)
    else:
        monkeypatch.setenv("AUGX_BLK", blk)
    species, opts = SHORTWIN_CFGS[cfg]
    return ax.Model(shortwin_config_path(), species, **opts)


@pytest.mark.parametrize("cfg", RUN_CFGS)
def test_decoder_is_created(monkeypatch, cfg):
    m = _model(monkeypatch, cfg)
    d = ax.Decoder(m, 0)
    r, = d.decode([random_dna(3000, 7500)])
    assert r.status == 0
    d.close()


def test_decoder_refuses_galdieria_with_utr_states(monkeypatch):
    m = _model(monkeypatch, "galdieria_utr")
    with pytest.raises(ax.AugxError) as e:
        ax.Decoder(m, 0)
    assert e.value.code == ax.AUGX_E_UNSUPPORTED


@pytest.mark.parametrize("blk", [None, "2"])
@pytest.mark.parametrize("cfg", RUN_CFGS)
def test_device_equals_twin_and_emulator(monkeypatch, cfg, blk):
    """Viterbi: every cell, ln V and the path equal the twin's; forward: every forward variable and ln P equal the emulator's, bit for
    bit; the batch in either order and decoded twice"""
    monkeypatch.setenv("AUGX_DEBUG_CELLS", "1")
    m = _model(monkeypatch, cfg, blk)
    S = m.n_states
    recs = shortwin_records(cfg)
    seqs = [s for _, s in recs]
    want = [twin_decode(m.tables_ptr, s, S, cells=True) for s in seqs]
    emu = emu_decode(m.tables_ptr, seqs, S, forward=True)
    d = ax.Decoder(m, 0)
    for order in (list(range(len(seqs))), list(range(len(seqs)))[::-1]):
        b = ax.Batch(d, [seqs[i] for i in order])
        for _ in range(2):
            b.decode()
            for k, (i, r) in enumerate(zip(order, b.paths())):
                rc, lnv, path, V, _ = want[i]
                assert r.status == rc == 0 and r.ln_viterbi == lnv and r.states == path, recs[i][0]
                assert np.array_equal(b.cells(k), V), recs[i][0]
        b.forward()
        worst = 0.0
        for k, i in enumerate(order):
            F, lnp = b.forward_cells(k)
            Fe, lnpe = emu[i][5], emu[i][6]
            assert np.array_equal(np.isfinite(F), np.isfinite(Fe)), recs[i][0]
            both = np.isfinite(F)
            worst = max(worst, float(np.max(np.abs(F[both] - Fe[both]))) if both.any() else 0.0, abs(lnp - lnpe))
        print("%s block %s: largest |ln F(device) - ln F(emulator)| = %.3g" % (cfg, blk or "chosen", worst))
        for k, i in enumerate(order):
            F, lnp = b.forward_cells(k)
            assert np.array_equal(F.view(np.uint64), emu[i][5].view(np.uint64)) and lnp == emu[i][6], recs[i][0]
        b.close()
    d.close()


@pytest.mark.parametrize("cfg", RUN_CFGS)
def test_device_samples_equal_the_emulators(monkeypatch, cfg):
    """99 sampled paths per record with the reference's generator, one stream over the records: the emulator's, draw for draw"""
    m = _model(monkeypatch, cfg)
    recs = [r for r in shortwin_records(cfg) if r[0] != "rand20k"]
    seqs = [s for _, s in recs]
    emu = emu_decode(m.tables_ptr, seqs, m.n_states, samples=99, seed=1)
    d = ax.Decoder(m, 0)
    res = ax.decode_sampled([d], seqs, 99, ax.Rand(1))
    for (name, _), (dec, smp), e in zip(recs, res, emu):
        assert dec.status == 0 and dec.ln_viterbi == e[1], name
        assert [[(b, en, t) for b, en, _, t in sp] for sp in smp] == e[7], name
    d.close()


@pytest.mark.parametrize("variant", [None] + list(VARIANTS))
@pytest.mark.parametrize("cfg", RUN_CFGS)
def test_executable_gff_equals_the_golden(tmp_path, cfg, variant):
    """the executable at the species' defaults (sample = 100), with --maxDNAPieceSize=9000 (the cut finder's exam windows; the motif
    records are cut at least twice), --softmasking=1, --singlestrand=true and --genemodel=complete: the reference binary's GFF"""
    fa = str(tmp_path / "x.fa")
    write_fasta(fa, variant_records(cfg, variant))
    env = dict(os.environ, AUGUSTUS_CONFIG_PATH=shortwin_config_path())
    env.pop("AUGX_BLK", None)
    args = ref_args(cfg, variant) + (["--progress=true"] if variant == "pieces" else [])
    ours = subprocess.run([EXE] + args + [fa], capture_output=True, text=True, env=env)
    assert ours.returncode == 0, ours.stderr[-2000:]
    gold = open(os.path.join(GOLDEN, "golden_shortwin_%s%s.gff" % (cfg, "_" + variant if variant else ""))).read().splitlines()
    assert gff_body(ours.stdout) == gold
    if variant == "pieces":  # (two cuts at least through the record with the motifs)
        assert sum(l.startswith("examining piece") for l in ours.stderr.splitlines()) >= 3 + len(variant_records(cfg, variant)) - 1
