"""--temperature=t (t = 0..7; reference Constant::temperature, LLDouble::heated): every forward summand and every option of a sampled
step carries its factor transition x emission raised to the power heat = (8 - t) / 8.  The device kernel bodies through the
lane-loop emulator and the host sampler against the REAL reference run live with the same option (CPU only; the same comparisons
run on the GPU in test_gpu_heated_sampling.py).  Every heated test fails when the heat is ignored: the cold matrix lies thousands
of ln units from the heated one (test_reference_heated_forward_is_far_from_cold)."""
import os
import re
import subprocess

import numpy as np
import pytest

import augustus_amd as ax
from helpers import *


def _forward_records():
    byname = dict(golden_inputs())
    return [(k, byname[k]) for k in ("HS04636", "HS08198", "rand20k_b", "withN", "short7", "short100", "short600", "iupac", "trunc_left",
                                     "trunc_right", "trunc_both", "revcomp", "softmask_rand")]


def _heated_records():
    # the single-class records of the cold forward tests and one record that runs through several GC classes
    return _forward_records() + gc_step_records(1, 4242)


def _close(name, F, fr, first=0):
    """the same cells alive and |ln F - ln F_ref| <= 1e-9 |ln F_ref| + 5e-9 (the bar of the cold forward tests); the largest
    deviation in units of the bar is returned (and printed by the callers)"""
    assert np.array_equal(np.isfinite(F[first:]), np.isfinite(fr[first:])), name
    both = np.isfinite(F) & np.isfinite(fr)
    dev, bar = np.abs(F[both] - fr[both]), 1e-9 * np.abs(fr[both]) + 5e-9
    worst = float((dev / bar).max()) if dev.size else 0.0
    print("%s: largest deviation %.3g (%.3g of the bar)" % (name, float(dev.max()) if dev.size else 0.0, worst))
    assert np.all(dev <= bar), (name, worst)
    return worst


S47 = {"human": ("human", {"softmasking": "0"}), "fly": ("fly", {"UTR": "off", "softmasking": "0"}),
       "arabidopsis": ("arabidopsis", {"UTR": "off", "softmasking": "0"})}


@needs_ref
@pytest.mark.parametrize("t", [1, 3, 4, 7])
@pytest.mark.parametrize("cfg", list(S47))
def test_emulated_heated_forward_matches_reference(tmp_path, cfg, t):
    """S = 47 (kernels.h: forwardPiece): every forward variable of the reference run with --temperature=t"""
    species, opts = S47[cfg]
    recs = _heated_records()
    fa = str(tmp_path / "f.fa")
    write_fasta(fa, recs)
    Fref = ref_forward(fa, species, ["--%s=%s" % kv for kv in opts.items()] + ["--temperature=%d" % t])
    m = ax.Model(config_path(), species, sample="100", temperature=str(t), **opts)
    res = emu_decode(m.tables_ptr, [s.upper() for _, s in recs], m.n_states, forward=True)
    for (name, seq), fr, r in zip(recs, Fref, res):
        _close(name, r[5], fr)


@needs_ref
@pytest.mark.parametrize("t", [1, 3, 4, 7])
@pytest.mark.parametrize("cfg", list(S47))
def test_reference_heated_forward_is_far_from_cold(tmp_path, cfg, t):
    """the comparison above can see the heat, on the same records: the reference's own heated matrix lies far from its cold one, so a
    harness that dropped the option could not pass.  Heating moves ln F by about t/8 of it: every cell of the last column whose
    |ln F_cold| t/8 is above 2 must lie more than 1 from the cold one (all records but the 7 bases of `short7`, ln F = -13, at
    t = 1), and every cell of every record more than 1e-3 -- 10^5 times the tolerance of the comparison"""
    species, opts = S47[cfg]
    recs = _heated_records()
    fa = str(tmp_path / "f.fa")
    write_fasta(fa, recs)
    extra = ["--%s=%s" % kv for kv in opts.items()]
    cold, hot = ref_forward(fa, species, extra), ref_forward(fa, species, extra + ["--temperature=%d" % t])
    far = 0
    for (name, seq), c, h in zip(recs, cold, hot):
        both = np.isfinite(c[-1]) & np.isfinite(h[-1])
        diff, expect = np.abs(c[-1][both] - h[-1][both]), np.abs(c[-1][both]) * t / 8
        print("%s: |ln F_cold - ln F_hot| of the last column %.3g .. %.3g" % (name, float(diff.min()), float(diff.max())))
        assert both.any() and np.all(diff > 1e-3) and np.all(diff[expect > 2.0] > 1.0), name
        far += bool(np.all(diff > 1.0))
    assert far >= len(recs) - 1


DENSE = [("human", {"UTR": "on", "softmasking": "0"}), ("fly", {}), ("human", {"genemodel": "exactlyone", "softmasking": "0"})]


@needs_ref
@pytest.mark.parametrize("t", [3, 7])
@pytest.mark.parametrize("species,opts", DENSE)
def test_emulated_heated_dense_forward_and_sampling_match_the_reference(tmp_path, species, opts, t):
    """the dense kernels (dense.h: densePiece<BLK, 1>; 71 states with --UTR=on, 48 with two intergenic states): every forward
    variable of the heated reference, and its sampled state paths draw for draw (the options of the host sampler, incl. the UTR
    exon candidates it evaluates itself, carry the same heat)"""
    m = ax.Model(config_path(), species, sample="100", temperature=str(t), **opts)
    S = m.n_states
    assert S in (71, 48)
    ex = dict(golden_inputs())
    names = ("HS04636", "HS08198", "short600", "trunc_both", "trunc_right", "iupac") if S == 71 else ("HS04636", "HS08198", "short600", "trunc_both", "iupac")
    recs = [(k, ex[k]) for k in names] + [("rnd", random_dna(12000, 77))]
    fa = str(tmp_path / "x.fa")
    write_fasta(fa, recs)
    extra = ["--%s=%s" % kv for kv in opts.items()] + ["--temperature=%d" % t]
    mats = ref_forward(fa, species, extra)
    smp = ref_samples(fa, species, extra, n=4)
    soft = opts.get("softmasking", "1") != "0"
    res = emu_decode(m.tables_ptr, [s if soft else s.upper() for _, s in recs], S, forward=True, samples=4)
    for (name, seq), R, rs, e in zip(recs, mats, smp, res):
        _close(name, e[5], R, first=1)
        assert [[tuple(x) for x in r] for r in rs] == [list(p) for p in e[7]], name


@needs_ref
@pytest.mark.parametrize("cfg", ["fly", "human1"])
def test_emulated_heated_sampling_matches_reference_paths(tmp_path, cfg):
    """S = 47, --temperature=3: 5 sampled paths per record, one generator over the records, equal to the reference's
    NAMGene::getSampledPath run live -- heated draw probabilities, and the heated thresholds of the runs down the chain states"""
    species, opts, _ = SAMPLED_CFGS[cfg]
    recs = sampled_records(cfg)
    fa = str(tmp_path / "x.fa")
    write_fasta(fa, recs)
    gold = ref_samples(fa, species, ["--%s=%s" % kv for kv in opts.items()] + ["--temperature=3"], n=5)
    m = ax.Model(config_path(), species, temperature="3", **opts)
    res = emu_decode(m.tables_ptr, [s.upper() for _, s in recs], m.n_states, samples=5)
    cold = golden_sampled_paths(cfg)
    differ = 0
    for (name, seq), r, g, c in zip(recs, res, gold, cold):
        assert len(g) == 5
        assert [list(p) for p in r[7]] == [[tuple(x) for x in q] for q in g], name
        differ += [[tuple(x) for x in q] for q in g] != c
    assert differ > 0  # (the heated sample is another one than the cold golden sample)


@needs_ref
@pytest.mark.parametrize("cfg", ["fly", "human1"])
def test_emulated_heated_gff_is_the_reference_binarys(tmp_path, cfg):
    """--sample=100 --temperature=3 --alternatives-from-sampling=true end to end on the CPU: emulator decode + heated forward + 99
    heated sampled paths per record, the host gene stage -> the GFF body of the reference binary run live, byte for byte (one record
    of the human set is set aside for the order of two equally probable alternatives, see below)"""
    species, opts, _ = SAMPLED_CFGS[cfg]
    opts = dict(opts, sample="100", temperature="3", **{"alternatives-from-sampling": "true"})
    recs = sampled_records(cfg)
    fa = str(tmp_path / "x.fa")
    write_fasta(fa, recs)
    ref = subprocess.run([REF_AUGUSTUS, "--AUGUSTUS_CONFIG_PATH=" + config_path(), "--species=" + species] +
                         ["--%s=%s" % kv for kv in opts.items()] + [fa], capture_output=True, text=True)
    assert ref.returncode == 0 and "# setting temperature to 3 (for sampling)" in ref.stdout.splitlines()
    m = ax.Model(config_path(), species, **opts)
    res = emu_decode(m.tables_ptr, [s.upper() for _, s in recs], m.n_states, samples=99)
    paths = [[(b, e, st, emu_state_type(m.tables_ptr, st)) for b, e, st in r[2]] for r in res]
    out, refl = format_gff_sampled(m, recs, paths, [r[7] for r in res]), gff_body(ref.stdout)

    def blocks(lines):  # record name -> the lines of its prediction block
        b, cur = {}, None
        for l in lines:
            if l.startswith("# ----- prediction on sequence number"):
                cur = l.split("name = ")[1].split(")")[0]
            b.setdefault(cur, []).append(l)
        return b
    bo, br = blocks(out), blocks(refl)
    assert list(bo) == list(br)
    # set aside: `trunc_left` under human -- two alternatives of gene g8 with EQUAL mean state probability come in the other order
    # (the known order-of-equals class, DESIGN.md section 6: the reference's order follows the addresses of its Gene objects); the
    # record's transcripts themselves, their coordinates and probabilities are compared with the numbering taken out
    aside = {"human1": ("trunc_left",)}.get(cfg, ())
    norm = lambda ls: sorted(re.sub(r"g(\d+)\.t\d+", r"g\1.tX", l) for l in ls if not l.startswith("#"))
    for name in bo:
        if name in aside:
            assert norm(bo[name]) == norm(br[name]) and len(bo[name]) == len(br[name]), name
        else:
            assert bo[name] == br[name], name


@pytest.mark.parametrize("species,opts", [("fly", {"UTR": "off", "softmasking": "0"}), ("human", {"UTR": "on", "softmasking": "0"})])
def test_cold_is_untouched(species, opts):
    """--temperature=0 is the default: the same forward matrix bit for bit and the same sampled paths as without the option, in both
    kernel families; and the Viterbi decode does not know the option at all (--temperature=3: the cold scores and paths)"""
    ex = dict(golden_inputs())
    recs = [(k, ex[k]) for k in ("HS04636", "short600", "trunc_both", "multigc_gene")]
    seqs = [s.upper() for _, s in recs]
    m = ax.Model(config_path(), species, sample="100", **opts)
    m0 = ax.Model(config_path(), species, sample="100", temperature="0", **opts)
    m3 = ax.Model(config_path(), species, sample="100", temperature="3", **opts)
    a = emu_decode(m.tables_ptr, seqs, m.n_states, forward=True, samples=4)
    b = emu_decode(m0.tables_ptr, seqs, m0.n_states, forward=True, samples=4)
    c = emu_decode(m3.tables_ptr, seqs, m3.n_states, forward=True, samples=4)
    for (name, _), x, y, z in zip(recs, a, b, c):
        assert np.array_equal(x[5], y[5]) and x[6] == y[6] and x[7] == y[7], name
        assert x[:3] == y[:3] == z[:3], name                      # status, ln Viterbi, Viterbi path
        assert not np.array_equal(x[5], z[5]), name


def test_temperature_above_7_is_the_heat_of_7():
    """--temperature=9 is clamped to 7: the forward matrix of t = 7, which is not the cold one (the note the reference prints for
    it: test_header_lines_of_the_executable below)"""
    seq = dict(golden_inputs())["short600"].upper()
    ms = [ax.Model(config_path(), "fly", UTR="off", softmasking="0", **o) for o in ({"temperature": "7"}, {"temperature": "9"}, {})]
    a, b, c = [emu_decode(m.tables_ptr, [seq], m.n_states, forward=True)[0] for m in ms]
    assert np.array_equal(a[5], b[5]) and not np.array_equal(b[5], c[5])
    both = np.isfinite(b[5][-1]) & np.isfinite(c[5][-1])
    assert np.all(np.abs(b[5][-1][both] - c[5][-1][both]) > 100)  # (600 bases at an eighth of the cold weight)


@pytest.mark.parametrize("value", ["abc", "3x", ""])
def test_temperature_that_is_no_number_is_refused(value):
    """a value that is not a whole number fails loudly: a run meant heated never comes out cold without a word"""
    with pytest.raises(Exception, match="temperature must be one of"):
        ax.Model(config_path(), "fly", temperature=value)


@pytest.mark.parametrize("t,line,note", [("3", "# setting temperature to 3 (for sampling)", ""), ("0", None, ""),
                                         ("9", "# setting temperature to 7 (for sampling)",
                                          "No temperature >7 allowed. temperature must be one of 0 1 2 3 4 5 6 7. Will use temperature=7.\n")])
def test_header_lines_of_the_executable(tmp_path, t, line, note):
    """the executable prints its header before it opens a device, so this runs without one: the reference's `# setting temperature`
    line right after the line that names the transition matrix (reference NAMGene::NAMGene, src/namgene.cc:139-140), none when
    cold, none with --/augustus/verbosity=0; the reference's note on the error stream above 7"""
    fa = str(tmp_path / "x.fa")
    write_fasta(fa, [("short600", dict(golden_inputs())["short600"])])
    env = dict(os.environ, AUGUSTUS_CONFIG_PATH=config_path())
    exe = os.path.join(ROOT, "augustus_amd", "bin", "augustus")
    base = [exe, "--species=fly", "--UTR=off", "--sample=0", "--temperature=" + t]
    r = subprocess.run(base + [fa], capture_output=True, text=True, env=env)
    lines = [l for l in r.stdout.splitlines() if not l.startswith("# " + exe)]
    at = [i for i, l in enumerate(lines) if "temperature" in l]
    if line is None:
        assert at == []
    else:
        assert [lines[i] for i in at] == [line] and lines[at[0] - 1].startswith("# fly version.")
    assert r.stderr.startswith(note) and ("temperature" in r.stderr) == bool(note)
    q = subprocess.run(base + ["--/augustus/verbosity=0", fa], capture_output=True, text=True, env=env)
    assert not any(l.startswith("# setting temperature") for l in q.stdout.splitlines())
