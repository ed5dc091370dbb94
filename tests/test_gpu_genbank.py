"""GenBank query files through the executable on the device: `augustus --species=X file.gb` predicts on every locus, prints the
annotation and ends with the accuracy report -- equal, byte for byte, to what the reference binary printed for the same command
(tests/golden/golden_genbank.json.gz, made by tests/golden/make_golden_genbank.py).  Compared is stdout from the line after
"# Looks like <file> is in genbank format." on (that line and the ones before it name the program and the paths of the run), without
the "# total time:" line (a clock) and the "# command line:" pair (paths), as aug_out_filter.pred of the reference's tests drops them;
and stderr, which is the reference's."""
import gzip
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

from helpers import *

EXE = os.path.join(ROOT, "augustus_amd", "bin", "augustus")
GB = os.path.join(GOLDEN, "genbank")


@pytest.fixture(scope="module")
def gold():
    return json.loads(gzip.open(os.path.join(GOLDEN, "golden_genbank.json.gz"), "rt").read())


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("genbank")
    for name in ("hsackI10.gb", "edge.gb"):
        open(str(d / name), "w").write(open(os.path.join(GB, name)).read())
    open(str(d / "fly12.gb"), "w").write(gzip.open(os.path.join(GB, "fly12.gb.gz"), "rt").read())
    return d


def filtered(stdout):
    lines = stdout.split("\n")
    i0 = [k for k, l in enumerate(lines) if l.startswith("# Looks like ")][0]
    assert lines[i0].endswith(" is in genbank format. Augustus uses the annotation for evaluation of accuracy.")
    out, skip, clock = [], False, 0
    for l in lines[i0 + 1:]:
        if skip:
            skip = False
            continue
        if l.startswith("# total time:"):
            assert float(l.split(":")[1]) > 0  # (a real clock reading)
            clock += 1
            continue
        if l.startswith("# command line:"):
            skip = True
            continue
        out.append(l)
    assert clock == 1
    return "\n".join(out)


_runs = {}


def run_case(inputs, c):
    key = (c["input"],) + tuple(c["args"])
    if key not in _runs:
        env = dict(os.environ, AUGUSTUS_CONFIG_PATH=config_path())
        _runs[key] = subprocess.run([EXE] + c["args"] + [str(inputs / c["input"])], capture_output=True, text=True, env=env)
    return _runs[key]


# the species' defaults on the three inputs (fly: UTR states, sample 100), and fly without either
@pytest.mark.parametrize("case", ["human_hsackI10", "human_edge", "fly_fly12", "fly_fly12_noutr_nosample", "fly_edge"])
def test_genbank_run_equals_the_reference(gold, inputs, case):
    c = gold["cases"][case]
    r = run_case(inputs, c)
    assert r.returncode == 0, r.stderr
    assert filtered(r.stdout) == c["stdout"]
    assert r.stderr == c["stderr"]


# the option variants, each on the smallest input that exercises it: GFF3 and one strand on the file with genes on both strands
# and UTR exons; soft-masking asked for (all of the input is lower case: the evidence blocks and the reference's warning);
# a cut through the annotated gene
@pytest.mark.parametrize("case", ["fly_edge_gff3", "fly_edge_forward", "human_hsackI10_softmasking", "human_hsackI10_cut"])
def test_genbank_option_variants(gold, inputs, case):
    c = gold["cases"][case]
    r = run_case(inputs, c)
    assert r.returncode == 0, r.stderr
    assert filtered(r.stdout) == c["stdout"]
    assert r.stderr == c["stderr"]


def prediction_lines(stdout):
    """per record the lines from "# Predicted genes for sequence number" up to the next block header or the report"""
    blocks, cur = [], None
    for l in stdout.split("\n"):
        if l.startswith("# Predicted genes for sequence number"):
            cur = []
            blocks.append(cur)
        elif l.startswith("# ----- ") or l in ("TSS distances ", "TTS distances ", "a-posteriori probability of viterbi path") or l.startswith("# command line:"):
            cur = None
        elif cur is not None and l != "#":
            cur.append(l)
    return blocks


def test_fasta_of_the_same_sequences_predicts_the_same(gold, inputs):
    """the mode changes nothing in the decode: the 12 sequences as FASTA with --softmasking=0 give the prediction lines of the
    GenBank run (gene numbers, posterior probabilities of the 100 sampled paths -- one stream of draws in input order -- included)"""
    c = gold["cases"]["fly_fly12"]
    gb = run_case(inputs, c)
    recs = []
    for entry in open(str(inputs / "fly12.gb")).read().split("\n//")[:-1]:
        name = entry[entry.index("LOCUS"):].split()[1]
        body = entry[entry.index("\nORIGIN"):].split("\n", 2)[2]
        recs.append((name, "".join(ch for ch in body if ch.isalpha())))
    assert len(recs) == 12
    fa = str(inputs / "fly12.fa")
    write_fasta(fa, recs)
    env = dict(os.environ, AUGUSTUS_CONFIG_PATH=config_path())
    r = subprocess.run([EXE, "--species=fly", "--softmasking=0", fa], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    ours_fa, ours_gb = prediction_lines(r.stdout), prediction_lines(gb.stdout)
    assert len(ours_fa) == len(ours_gb) == 12 and sum(len(b) for b in ours_fa) > 300
    assert ours_fa == ours_gb
