"""GenBank query files on the host: the reader (augustus_amd/csrc/genbank.cc), the printed annotation and the accuracy report
(augustus_amd/csrc/evaluation.cc) against what the reference binary printed for the same inputs (tests/golden/golden_genbank.json.gz,
made by tests/golden/make_golden_genbank.py), and the errors.  No device is needed for any of it; the executable's refusals and its
"not recognized" error come before it asks for one."""
import gzip
import json
import os
import re
import subprocess

import pytest

import augustus_amd as ax
from helpers import *

EXE = os.path.join(ROOT, "augustus_amd", "bin", "augustus")
GB = os.path.join(GOLDEN, "genbank")
BLOCKS = ("hsackI10_human", "edge_human", "edge_fly", "edge_fly_forward", "fly12_fly")


def gb_text(name):
    p = os.path.join(GB, name)
    return open(p).read() if os.path.exists(p) else gzip.open(p + ".gz", "rt").read()


@pytest.fixture(scope="module")
def gold():
    return json.loads(gzip.open(os.path.join(GOLDEN, "golden_genbank.json.gz"), "rt").read())


def origin_sequences(text):
    """(LOCUS name, LOCUS length, the letters after ORIGIN) of every entry, read the plain way"""
    out = []
    for entry in text.split("\n//")[:-1]:
        head = re.search(r"^LOCUS\s+(\S+)\s+(\d+) bp", entry, re.M)
        body = entry[re.search(r"^ORIGIN.*$", entry, re.M).end():]
        out.append((head.group(1), int(head.group(2)), "".join(c for c in body if c.isalpha())))
    return out


def read_for(species, text, **opts):
    """the file read as the executable reads it for this species and these options"""
    m = ax.Model(config_path(), species, softmasking="0", **opts)
    return ax.GenBank(text, utr=m.option("UTR") in ("both", "1", "on", "5"), stop_excluded=m.option("stopCodonExcludedFromCDS") in ("true", "1", "on", "yes"))


@pytest.mark.parametrize("key", BLOCKS)
def test_reader_and_printed_annotation(gold, key):
    b = gold["blocks"][key]
    text = gb_text(b["input"])
    assert ax.input_type(text) == ax.INPUT_GENBANK
    g = read_for(b["species"], text)
    want = origin_sequences(text)
    assert len(g) == len(want) == len(b["loci"])
    assert g.stderr == b["reader_stderr"]
    for fmt, opts in (("annotation", {}), ("annotation_gff3", {"gff3": "on"})):
        m = ax.Model(config_path(), b["species"], softmasking="0", **opts)
        for i, (name, length, seq) in enumerate(want):
            gname, gseq, glen, txs = g.locus(i)
            assert (gname, glen, gseq) == (name, length, seq) and [gname, glen] == b["loci"][i]
            assert len(txs) == len(set(re.findall(r'transcript_id "([^"]+)"|Parent=(\S+)', b[fmt][i])))
            assert g.annotation_gff(m, i) == b[fmt][i], (key, fmt, i)


def test_reader_flat_transcripts():
    """the flat form of the edge file's genes: strands, kinds, frames, partial ends, the names the reference gives"""
    g = ax.GenBank(gb_text("edge.gb"), utr=True)
    loci = [g.locus(i) for i in range(len(g))]
    assert [len(l[3]) for l in loci] == [2, 1, 1, 1, 0, 1, 1]
    a, b = loci[0][3]
    assert (a["gene_id"], a["strand"], b["gene_id"], b["strand"]) == ("edgeA", -1, "edgeB", 1)
    assert [(e[0], e[1], e[2]) for e in a["exons"]] == [(1593, 1649, ax.EXON_UTR5), (765, 901, ax.EXON_CDS), (962, 1592, ax.EXON_CDS),
                                                         (599, 649, ax.EXON_UTR3), (699, 764, ax.EXON_UTR3)]
    assert (a["trans_start"], a["trans_end"], a["coding_start"], a["coding_end"]) == (599, 1649, 765, 1592)
    assert [e[4] for e in b["exons"]] == [0] and b["exons"][0][:3] == (1699, 1899, ax.EXON_CDS)
    assert (loci[1][3][0]["complete_left"], loci[1][3][0]["complete_right"]) == (0, 1)
    c = loci[2][3][0]
    assert (c["complete_left"], c["complete_right"], c["complete_5utr"], c["complete_3utr"]) == (1, 0, 1, 0) and c["gene_id"] == "chr2L_2765909-2767213-1"
    assert loci[3][3][0]["strand"] == -1 and len(loci[3][3][0]["exons"]) == 1
    # the mRNA of another gene name does not pair with the CDS (no UTR exon), and as it overlaps the CDS it is no gene of its own
    assert [(t["gene_id"], {e[2] for e in t["exons"]}) for t in loci[5][3]] == [("edgeD", {ax.EXON_CDS})]
    assert "CDS edgeF out of range. Ignoring it.\n" in g.stdout and g.stdout.endswith("# Read in 7 genbank sequences.\n")
    # without --UTR the mRNA features are not read
    g0 = ax.GenBank(gb_text("edge.gb"), utr=False)
    assert all(e[2] == ax.EXON_CDS for i in range(len(g0)) for t in g0.locus(i)[3] for e in t["exons"])


@pytest.mark.parametrize("key", BLOCKS)
def test_evaluation_report(gold, key):
    """the reference's predicted transcripts and the parsed annotation through the evaluation entries: the reference's report"""
    b = gold["blocks"][key]
    g = read_for(b["species"], gb_text(b["input"]))
    ev = ax.Evaluation()
    strand = 1 if "--strand=forward" in b["args"] else 0
    for i in range(len(g)):
        ev.add(b["predicted"][i], g.locus(i)[3], strand)
    assert ev.report() == b["report"]


def test_evaluation_of_one_strand(gold):
    """--strand=forward: the genes of the reverse strand are left out on both sides"""
    n_anno = lambda rep: int(re.search(r"^exon level \|\s+\d+ \|\s+(\d+) \|", rep, re.M).group(1))
    assert n_anno(gold["blocks"]["edge_fly_forward"]["report"]) < n_anno(gold["blocks"]["edge_fly"]["report"]) == 13


@pytest.mark.parametrize("key", BLOCKS)
def test_annotation_as_prediction_is_perfect(gold, key):
    b = gold["blocks"][key]
    g = read_for(b["species"], gb_text(b["input"]))
    ev = ax.Evaluation()
    for i in range(len(g)):
        txs = g.locus(i)[3]
        ev.add(txs, txs)
    rep = ev.report()
    vals = re.findall(r"^(nucleotide level|exon level|gene level| UTR exon level| UTR base level) \|(?:.*\|)?\s+(\S+) \|\s+(\S+) \|$", rep, re.M)
    assert len(vals) >= 3
    for what, sens, spec in vals:
        assert sens in ("1", "-nan") and spec in ("1", "-nan"), (what, sens, spec)
    assert [v[1:] for v in vals[:3]] == [("1", "1")] * 3
    assert re.search(r"^\s+\|\s+\|\s+\|\s+\|\s+0 \|\s+0 \|", rep, re.M)  # no false positive, no false negative exon


# ---- errors -----------------------------------------------------------------------------------------------------------------

HS = None


def hs():
    global HS
    HS = HS or gb_text("hsackI10.gb")
    return HS


def test_truncated_file_has_no_complete_entry():
    """an entry without its "//" line is not read (reference GBSplitter::gotoEnd); with no other entry: the reference's error"""
    cut = hs()[:len(hs()) // 2]
    assert ax.input_type(cut) == ax.INPUT_GENBANK
    with pytest.raises(ax.AugxError) as e:
        ax.GenBank(cut)
    assert e.value.code == -2 and "No genbank sequences found." in str(e.value)
    # a complete entry followed by half of one: the complete one is read
    g = ax.GenBank(hs() + cut)
    assert len(g) == 1 and g.stdout == "# Read in 1 genbank sequences.\n"


def test_entry_without_origin_is_refused_by_name():
    text = hs()
    k = text.index("ORIGIN")
    no_origin = text[:k] + "//\n"
    assert ax.input_type(no_origin + text) == ax.INPUT_GENBANK
    g = ax.GenBank(no_origin + text)
    assert len(g) == 1
    assert g.stderr.startswith("GBProcessor::getGeneList(): No 'ORIGIN' line in the entry: no sequence.\nEncountered error after reading 0 annotations.\n")
    with pytest.raises(ax.AugxError) as e:
        ax.GenBank(no_origin)
    assert "No genbank sequences found." in str(e.value)


def test_feature_past_the_end_and_other_reader_errors():
    text = hs()
    # a CDS past the end: ignored with the reference's line on the output stream; the locus then has no gene
    far = re.sub(r"join\(1674\.\.2300", "join(1674..2300,9000..9100", text, count=1)
    assert far != text
    g = ax.GenBank(far)
    assert g.stdout == "CDS  out of range. Ignoring it.\n# Read in 1 genbank sequences.\n" and g.locus(0)[3] == []
    assert g.stderr == "No 'CDS' found in sequence HSACKI10\nNo correct 'CDS' found in sequence HSACKI10\n"
    # exons out of order: the locus is dropped with the reference's lines
    swapped = text.replace("join(1674..2300,3142..3224", "join(3142..3224,1674..2300", 1)
    assert swapped != text
    with pytest.raises(ax.AugxError) as e:
        ax.GenBank(swapped)
    assert "One CDS exon does not begin properly after the previous CDS exon.3223 >= 1673" in str(e.value)
    assert "GBProcessor::getGeneList(): Intron has non-positive length.\nEncountered error after reading 0 annotations.\n" in str(e.value)
    # an operator inside join(): refused, naming the character the reference names
    nested = text.replace("join(1674..2300,", "join(complement(1674..2300),", 1)
    with pytest.raises(ax.AugxError) as e:
        ax.GenBank(nested)
    assert "CDS contains character c\nGBProcessor::getGeneList(): GBProcessor::getJoin( ):  failed!!!" in str(e.value)
    # more bases than the source line says
    longer = text.replace("source          1..6483", "source          1..6000", 1)
    with pytest.raises(ax.AugxError) as e:
        ax.GenBank(longer)
    assert "Sequence was longer than the expected 6000 bp." in str(e.value)
    # fewer: a warning, and the length is the number of bases
    g = ax.GenBank(text.replace("source          1..6483", "source          1..7000", 1))
    assert g.locus(0)[2] == 6483 and "Warning: Sequence was shorter than expected frome the source line of the Genbank entry ( expected 7000 bp)" in g.stderr


def run_exe(args, **kw):
    env = dict(os.environ, AUGUSTUS_CONFIG_PATH=config_path())
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=env, **kw)


def test_neither_format_keeps_its_error(tmp_path):
    fn = str(tmp_path / "x.txt")
    open(fn, "w").write("12 34\nLOCUS but no sequence line\n")
    assert ax.input_type(open(fn).read()) == ax.INPUT_UNKNOWN
    r = run_exe(["--species=human", fn])
    assert r.returncode == 1
    assert r.stderr.endswith("ERROR\n\tFile format of " + fn + " not recognized (only FASTA input is supported on the MI355X path).\n\n")


@pytest.mark.parametrize("opt", ["noprediction", "checkExAcc"])
def test_training_and_hints_options_are_refused_by_name(tmp_path, opt):
    fn = os.path.join(GB, "hsackI10.gb")
    r = run_exe(["--species=human", "--%s=true" % opt, fn])
    assert r.returncode == 1 and r.stdout == ""
    assert ("--%s=true" % opt) in r.stderr and "outside the MI355X ab-initio hot path" in r.stderr
    # the entry that writes the report refuses them with AUGX_E_UNSUPPORTED
    m = ax.Model(config_path(), "human", softmasking="0", **{opt: "true"})
    with pytest.raises(ax.AugxError) as e:
        ax.GenBank(hs()).report(m, [])
    assert e.value.code == ax.AUGX_E_UNSUPPORTED and opt in str(e.value)


# ---- the whole path without a device: the emulator decodes, the product writes the output --------------------------------------

def emulated_report(species, text, **opts):
    m = ax.Model(config_path(), species, softmasking="0", **opts)
    g = read_for(species, text, **opts)
    S = m.n_states
    loci = [g.locus(i) for i in range(len(g))]
    res = emu_decode(m.tables_ptr, [l[1] for l in loci], S)
    tys = [emu_state_type(m.tables_ptr, s) for s in range(S)]
    pieces = [(i, 0, len(l[1]) - 1, r[0], [(b, e, s, tys[s]) for b, e, s in r[2]]) for i, (l, r) in enumerate(zip(loci, res))]
    return g.stdout + g.report(m, pieces)


def drop_clock_and_command(stdout):
    lines, out, skip = stdout.split("\n"), [], False
    i0 = [k for k, l in enumerate(lines) if l.startswith("# Looks like ")]
    for l in lines[i0[0] + 1 if i0 else 0:]:
        if skip or l.startswith("# total time:"):
            skip = False
            continue
        if l.startswith("# command line:"):
            skip = True
            continue
        out.append(l)
    return "\n".join(out)


@pytest.mark.parametrize("inp", ["hsackI10.gb", "edge.gb"])
def test_emulated_run_equals_the_golden(gold, inp):
    c = gold["cases"]["human_" + inp[:-3]]
    assert drop_clock_and_command(emulated_report("human", gb_text(inp))) == c["stdout"]


@needs_ref
@pytest.mark.parametrize("inp,opts", [("hsackI10.gb", {}), ("edge.gb", {}), ("edge.gb", {"gff3": "on", "strand": "backward"}), ("edge.gb", {"stopCodonExcludedFromCDS": "true", "exonnames": "on"})])
def test_emulated_run_equals_the_live_reference(tmp_path, inp, opts):
    fn = str(tmp_path / inp)
    open(fn, "w").write(gb_text(inp))
    ref = subprocess.run([REF_AUGUSTUS, "--AUGUSTUS_CONFIG_PATH=" + config_path(), "--species=human"] + ["--%s=%s" % kv for kv in opts.items()] + [fn],
                         capture_output=True, text=True)
    assert ref.returncode == 0
    ours = emulated_report("human", gb_text(inp), **opts)
    assert drop_clock_and_command(ours) == drop_clock_and_command(ref.stdout)
