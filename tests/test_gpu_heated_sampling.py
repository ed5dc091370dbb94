"""GPU parity of --temperature (heated forward pass and heated path sampling): the device forward matrix of both kernel families
against the REAL reference run live with the same option, the executable against golden files of the reference binary
(tests/golden/make_golden_heated.py), the sampled paths of the C ABI against golden paths.  Every test here but the last fails when
the heat is ignored: the output is then the cold one."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import augustus_amd as ax
from helpers import *

EXE = os.path.join(ROOT, "augustus_amd", "bin", "augustus")
HEATED_CFGS = ("fly", "fly_alt", "human1_sm", "human_utr_alt")  # (tests/golden/make_golden_heated.py)


def _forward_against_reference(tmp_path, species, opts, recs, t, first):
    fa = str(tmp_path / "f.fa")
    write_fasta(fa, recs)
    Fref = ref_forward(fa, species, ["--%s=%s" % kv for kv in opts.items()] + ["--temperature=%d" % t])
    m = ax.Model(config_path(), species, sample="100", temperature=str(t), **opts)
    d = ax.Decoder(m, 0)
    b = ax.Batch(d, [s for _, s in recs])
    b.decode()
    b.forward()
    for i, ((name, seq), fr, r) in enumerate(zip(recs, Fref, b.paths())):
        if r.status != 0:
            continue
        F, lnp = b.forward_cells(i)
        assert np.array_equal(np.isfinite(F[first:]), np.isfinite(fr[first:])), name
        both = np.isfinite(F) & np.isfinite(fr)
        dev, bar = np.abs(F[both] - fr[both]), 1e-9 * np.abs(fr[both]) + 5e-9
        print("%s: largest deviation %.3g (%.3g of the bar)" % (name, float(dev.max()), float((dev / bar).max())))
        assert np.all(dev <= bar), name


@needs_ref
@pytest.mark.parametrize("t", [3, 7])
@pytest.mark.parametrize("cfg", ["human_nosm", "fly"])
def test_gpu_heated_forward_matches_reference(tmp_path, cfg, t):
    """kForward (S = 47) with --temperature=t against every forward variable of the heated reference: the same cells alive, ln F
    within 1e-9 relative; human: incl. the pieces with several GC classes (transition terms from HBM, scaled where they are used)"""
    species, opts = GOLDEN_CFGS[cfg]
    byname = dict(golden_inputs())
    recs = [(k, byname[k]) for k in ("HS04636", "HS08198", "rand20k_b", "withN", "short7", "short100", "short600", "iupac", "trunc_left",
                                     "trunc_right", "trunc_both", "revcomp", "softmask_rand", "rand60k")]
    if cfg == "human_nosm":
        recs += [(k, byname[k]) for k in ("multigc_gene", "multigc_two", "multigc_rand", "multigc_levels")]
    _forward_against_reference(tmp_path, species, {k: v for k, v in opts.items() if k != "sample"}, recs, t, 0)


@needs_ref
@pytest.mark.parametrize("t", [3, 7])
@pytest.mark.parametrize("species,opts,multi", [("fly", {}, False), ("human", {"UTR": "on", "softmasking": "0"}, True),
                                                ("human", {"genemodel": "exactlyone", "softmasking": "0"}, True)])
def test_gpu_heated_dense_forward_matches_reference(tmp_path, species, opts, multi, t):
    """kDense<BLK, 1> (S = 71 / 48) with --temperature=t against the heated reference, incl. records with several GC classes"""
    ex = dict(golden_inputs())
    names = ["HS04636", "HS08198", "short600", "trunc_both", "trunc_right", "iupac"] + (["multigc_gene", "multigc_rand", "multigc_two", "multigc_levels"] if multi else [])
    recs = [(k, ex[k]) for k in names] + [("rnd", random_dna(12000, 77))]
    _forward_against_reference(tmp_path, species, opts, recs, t, 1)


def _heated_cli(tmp_path, cfg, temperature="3"):
    species, opts, _ = SAMPLED_CFGS[cfg]
    fa = str(tmp_path / "in.fa")
    write_fasta(fa, sampled_records(cfg))
    env = dict(os.environ, AUGUSTUS_CONFIG_PATH=config_path())
    return subprocess.run([EXE, "--species=" + species] + ["--%s=%s" % kv for kv in opts.items()] + ["--temperature=" + temperature, fa],
                          capture_output=True, text=True, env=env)


def _no_cmdline(out):
    return [l for l in out.splitlines() if not l.startswith("# command line") and not l.startswith("# " + EXE)]  # (and its echo)


@pytest.mark.parametrize("cfg", HEATED_CFGS)
def test_cli_heated_gff_identical_to_reference(tmp_path, cfg):
    """the executable with --temperature=3 and sampling on (fly, fly with --alternatives-from-sampling=true, human with the
    soft-masking bonus, human with UTR states and alternatives): the GFF byte-identical to the reference binary's, and the header line
    the reference prints for the option, where it prints it (after the line that names the transition matrix)"""
    r = _heated_cli(tmp_path, cfg)
    assert r.returncode == 0, r.stderr
    assert gff_body(r.stdout) == open(os.path.join(GOLDEN, "golden_heated_%s.gff" % cfg)).read().splitlines()
    lines = r.stdout.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("# setting temperature")]
    assert [lines[i] for i in at] == open(os.path.join(GOLDEN, "golden_heated_%s.head" % cfg)).read().splitlines()
    assert lines[at[0] - 1].startswith("# %s version." % SAMPLED_CFGS[cfg][0])
    assert r.stderr == ""


@pytest.mark.parametrize("cfg", ["fly", "human1_sm", "human_utr_alt"])
def test_heated_sampled_paths_are_the_references(cfg):
    """augx_decode_sampled with a heated model: 5 sampled paths per record, one generator over the records -> the paths of the
    reference's NAMGene::getSampledPath under --temperature=3, state by state"""
    species, opts, _ = SAMPLED_CFGS[cfg]
    recs = sampled_records(cfg)
    g = json.load(open(os.path.join(GOLDEN, "golden_heated_paths_%s.json" % cfg)))
    gold = [[[tuple(st) for st in smp] for smp in r["samples"]] for r in g["records"]]
    m = ax.Model(config_path(), species, temperature="3", **opts)
    d = ax.Decoder(m)
    soft = opts.get("softmasking", "1") != "0"
    res = ax.decode_sampled([d], [s if soft else s.upper() for _, s in recs], 5, ax.Rand(1))
    for (name, _), (dec, smp), gp in zip(recs, res, gold):
        assert dec.status == 0, name
        assert [[(b, e, t) for b, e, _, t in sp] for sp in smp] == gp, name
    assert gold != golden_sampled_paths(cfg)


def test_cli_temperature_above_7(tmp_path):
    """--temperature=9: the reference's line on the error stream, and the output of --temperature=7"""
    r9, r7 = _heated_cli(tmp_path, "fly", "9"), _heated_cli(tmp_path, "fly", "7")
    assert r9.returncode == 0 and r7.returncode == 0
    assert r9.stderr == "No temperature >7 allowed. temperature must be one of 0 1 2 3 4 5 6 7. Will use temperature=7.\n" and r7.stderr == ""
    assert "# setting temperature to 7 (for sampling)" in r9.stdout.splitlines()
    assert _no_cmdline(r9.stdout) == _no_cmdline(r7.stdout)
    assert gff_body(r7.stdout) != golden_sampled_gff("fly")


def test_cli_cold_is_untouched(tmp_path):
    """--temperature=0 is the default (the cold golden GFF, no header line); --temperature=3 --sample=0 gives the cold Viterbi GFF
    plus the one header line: the Viterbi decode does not know the option"""
    r0 = _heated_cli(tmp_path, "fly", "0")
    assert r0.returncode == 0 and gff_body(r0.stdout) == golden_sampled_gff("fly")
    assert not any("temperature" in l for l in _no_cmdline(r0.stdout))
    fa = str(tmp_path / "in.fa")
    env = dict(os.environ, AUGUSTUS_CONFIG_PATH=config_path())
    base = [EXE, "--species=fly", "--UTR=off", "--softmasking=0", "--sample=0"]
    a = subprocess.run(base + [fa], capture_output=True, text=True, env=env)
    b = subprocess.run(base + ["--temperature=3", fa], capture_output=True, text=True, env=env)
    assert a.returncode == 0 and b.returncode == 0
    assert [l for l in _no_cmdline(b.stdout) if l != "# setting temperature to 3 (for sampling)"] == _no_cmdline(a.stdout)
    assert len(_no_cmdline(b.stdout)) == len(_no_cmdline(a.stdout)) + 1
