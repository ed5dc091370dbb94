#!/usr/bin/env python3
"""Goldens from the REAL reference (oracle/_ref, built by oracle/Makefile) for runs on GenBank input: prediction, the printed
annotation and the accuracy report (reference evaluateOnTestSet, src/augustus.cc:254-364).  Run where the reference's sources
lie (REF, as in oracle/Makefile):  python tests/golden/make_golden_genbank.py

Inputs (tests/golden/genbank/, data the reference's programs read):
  hsackI10.gb   examples/hsackI10.gb: one human locus of 6 483 bases
  fly12.gb.gz   the first 12 loci of examples/chr2L/genes.gb.test
  edge.gb       seven short loci of examples/chr2L/genes.gb.test (none among the first 12) whose feature tables are written by
                hand below: EDGE
Outputs: golden_genbank.json.gz
  cases[name]   = {input, args, stdout, stderr}: the reference binary's output streams.  stdout from the line after "# Looks like <file>
                  is in genbank format." on (that line and what precedes it name the program and the paths of the run), without the "# total time:" line
                  (a clock) and the "# command line:" pair (paths) -- what aug_out_filter.pred of the reference's tests drops, too
  blocks[key]   = per input, species and strand option: names and lengths of the loci, the "# annotation:" blocks in GFF and GFF3, the report, and
                  the reference's predicted transcripts as exon lists (read off a second run with --print_utr=on --tss=on --tts=on)
"""
import gzip
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from helpers import REF_AUGUSTUS, config_path  # noqa

REF = os.environ.get("REF", "/root/reference")
GB = os.path.join(HERE, "genbank")

# ---- the edge file: locus of genes.gb.test -> the lines of its feature table after `source`
EDGE = [
    # a reverse-strand gene with an mRNA around it (two 3'UTR exons left of the CDS, one 5'UTR exon right of it) and a second,
    # single-exon gene on the forward strand in the same locus
    ("chr2L_817742-819706", """\
     mRNA            complement(join(600..650,700..902,963..1650))
                     /gene="edgeA"
     CDS             complement(join(766..902,963..1593))
                     /gene="edgeA"
     CDS             1700..1900
                     /gene="edgeB"
"""),
    # a CDS partial at its 5' end
    ("chr2L_1980930-1982119", """\
     CDS             join(<318..654,713..903,957..998)
                     /gene="edgeC"
"""),
    # a CDS partial at its 3' end, with an mRNA that is partial there too
    ("chr2L_2765909-2767213", """\
     mRNA            join(350..799,859..>1182)
     CDS             join(407..799,859..>1182)
"""),
    # a single-exon gene on the reverse strand; no /gene= (the reference names it after the locus)
    ("chr2L_2226377-2227042", """\
     CDS             complement(172..639)
"""),
    # a locus without a gene
    ("chr2L_2225520-2226376", ""),
    # a gene with a stop codon in frame (second exon moved by one base); an mRNA with another name, which therefore does not pair
    ("chr2L_2879112-2880849", """\
     mRNA            join(100..768,934..1500)
                     /gene="other"
     CDS             join(153..768,934..1360)
                     /gene="edgeD"
"""),
    # annotated exons that overlap the ones a gene finder sees here without sharing an end with them (the true gene is
    # join(102..962,1028..1777)), and a feature past the end of the sequence, which the reference ignores with a line on its output
    ("chr2L_811535-814697", """\
     CDS             join(150..900,1060..1700)
                     /gene="edgeE"
     CDS             join(2500..2600,3100..3200)
                     /gene="edgeF"
"""),
]

CASES = {
    # name: (input, arguments)
    "human_hsackI10": ("hsackI10.gb", ["--species=human"]),
    "human_edge": ("edge.gb", ["--species=human"]),
    "fly_fly12": ("fly12.gb", ["--species=fly"]),
    "fly_fly12_noutr_nosample": ("fly12.gb", ["--species=fly", "--UTR=off", "--sample=0"]),
    "fly_edge": ("edge.gb", ["--species=fly"]),
    "fly_edge_gff3": ("edge.gb", ["--species=fly", "--gff3=on"]),
    "fly_edge_forward": ("edge.gb", ["--species=fly", "--strand=forward"]),
    "human_hsackI10_softmasking": ("hsackI10.gb", ["--species=human", "--softmasking=1"]),
    "human_hsackI10_cut": ("hsackI10.gb", ["--species=human", "--predictionStart=2500", "--predictionEnd=5200"]),
}
# key: (input, species, further arguments)
BLOCKS = {"hsackI10_human": ("hsackI10.gb", "human", []), "edge_human": ("edge.gb", "human", []), "edge_fly": ("edge.gb", "fly", []),
          "edge_fly_forward": ("edge.gb", "fly", ["--strand=forward"]), "fly12_fly": ("fly12.gb", "fly", [])}


def split_loci(text):
    out, cur = [], []
    for l in text.splitlines(True):
        cur.append(l)
        if l.startswith("//"):
            out.append("".join(cur))
            cur = []
    return out


def make_inputs():
    os.makedirs(GB, exist_ok=True)
    shutil.copy(os.path.join(REF, "examples", "hsackI10.gb"), os.path.join(GB, "hsackI10.gb"))
    loci = split_loci(open(os.path.join(REF, "examples", "chr2L", "genes.gb.test")).read())
    with gzip.GzipFile(os.path.join(GB, "fly12.gb.gz"), "wb", mtime=0) as f:
        f.write("".join(loci[:12]).encode())
    by_name = {l.split()[1]: l for l in loci[12:]}
    edge = []
    for name, table in EDGE:
        lines = by_name[name].splitlines(True)
        i0 = [k for k, l in enumerate(lines) if l.startswith("     source")][0]
        i1 = [k for k, l in enumerate(lines) if l.startswith("BASE COUNT") or l.startswith("ORIGIN")][0]
        edge.append("".join(lines[:i0 + 1]) + table + "".join(lines[i1:]))
    open(os.path.join(GB, "edge.gb"), "w").write("".join(edge))


def read_input(name):
    p = os.path.join(GB, name)
    return gzip.open(p + ".gz", "rt").read() if not os.path.exists(p) else open(p).read()


def run_ref(d, inp, args):
    fn = os.path.join(d, inp)
    if not os.path.exists(fn):
        open(fn, "w").write(read_input(inp))
    r = subprocess.run([REF_AUGUSTUS, "--AUGUSTUS_CONFIG_PATH=" + config_path()] + args + [inp], capture_output=True, text=True, cwd=d)
    return r.returncode, r.stdout, r.stderr


def filter_out(stdout):
    """from the line after "# Looks like <file> is in genbank format." on, without the clock and the echo of the command"""
    lines = stdout.split("\n")
    i0 = [k for k, l in enumerate(lines) if l.startswith("# Looks like ")][0] + 1
    out, skip = [], False
    for l in lines[i0:]:
        if skip:
            skip = False
            continue
        if l.startswith("# total time:"):
            continue
        if l.startswith("# command line:"):
            skip = True
            continue
        out.append(l)
    return "\n".join(out)


def annotation_blocks(stdout):
    """the text between "# annotation: " and "# Predicted genes" of every locus, and (name, length) of the headers"""
    blocks, heads, cur = [], [], None
    for l in stdout.split("\n"):
        m = re.match(r"# ----- sequence number \d+ \(length = (\d+), name = (.*)\) -----$", l)
        if m:
            heads.append((m.group(2), int(m.group(1))))
        if l == "# annotation: ":
            cur = []
        elif l.startswith("# Predicted genes for sequence number") and cur is not None:
            blocks.append("".join(x + "\n" for x in cur))
            cur = None
        elif cur is not None:
            cur.append(l)
    return heads, blocks


def report_block(stdout):
    lines = stdout.split("\n")
    i0 = min(k for k, l in enumerate(lines) if l in ("TSS distances ", "TTS distances ", "a-posteriori probability of viterbi path"))
    i1 = [k for k, l in enumerate(lines) if l.startswith("# total time:")][0]
    return "".join(x + "\n" for x in lines[i0:i1])


def predicted_transcripts(stdout):
    """per locus the predicted transcripts of a run with --print_utr=on --tss=on --tts=on, in the flat form of augx_transcript"""
    loci, cur, tx = [], None, None
    for l in stdout.split("\n"):
        if l.startswith("# Predicted genes for sequence number"):
            cur = []
            loci.append(cur)
            continue
        f = l.split("\t")
        if cur is None or len(f) < 9 or f[1] != "AUGUSTUS":
            continue
        b, e = int(f[3]) - 1, int(f[4]) - 1
        if f[2] == "transcript":
            tx = {"strand": 1 if f[6] == "+" else -1, "exons": [], "tb": b, "te": e, "start": False, "stop": False, "tss": False, "tts": False, "id": f[8]}
            cur.append(tx)
        elif f[2] == "CDS":
            tx["exons"].append((b, e, 0))
        elif f[2] in ("5'-UTR", "3'-UTR"):
            tx["exons"].append((b, e, 1 if f[2][0] == "5" else 2))
        elif f[2] in ("start_codon", "stop_codon", "tss", "tts"):
            tx[f[2].split("_")[0]] = True
    for txs in loci:
        for t in txs:
            cds = [x for x in t["exons"] if x[2] == 0]
            t["coding_start"], t["coding_end"] = min(x[0] for x in cds), max(x[1] for x in cds)
            t["trans_start"] = t["tb"] if t["tb"] != t["coding_start"] else -1
            t["trans_end"] = t["te"] if t["te"] != t["coding_end"] else -1
            t["complete"] = int(t["start"] and t["stop"])
            t["complete_5utr"] = int(t["tss"] or not any(x[2] == 1 for x in t["exons"]))
            t["complete_3utr"] = int(t["tts"] or not any(x[2] == 2 for x in t["exons"]))
            t["exons"] = sorted(x for x in t["exons"] if x[2] == 1) + sorted(cds) + sorted(x for x in t["exons"] if x[2] == 2)
            for k in ("tb", "te", "start", "stop", "tss", "tts"):
                del t[k]
    return loci


def main():
    make_inputs()
    d = tempfile.mkdtemp()
    gold = {"cases": {}, "blocks": {}}
    for name, (inp, args) in CASES.items():
        rc, out, err = run_ref(d, inp, args)
        assert rc == 0, (name, err[-2000:])
        gold["cases"][name] = {"input": inp, "args": args, "stdout": filter_out(out), "stderr": err}
        print(name, len(out.splitlines()), "lines;", "stderr:", repr(err[:300]))
    for key, (inp, species, more) in BLOCKS.items():
        rc, out, err = run_ref(d, inp, ["--species=" + species] + more)
        rc3, out3, _ = run_ref(d, inp, ["--species=" + species, "--gff3=on"] + more)
        rcu, outu, _ = run_ref(d, inp, ["--species=" + species, "--print_utr=on", "--tss=on", "--tts=on"] + more)
        assert rc == 0 and rc3 == 0 and rcu == 0
        heads, anno = annotation_blocks(out)
        _, anno3 = annotation_blocks(out3)
        assert report_block(out) == report_block(outu)  # (the output options change nothing in the prediction)
        gold["blocks"][key] = {"input": inp, "species": species, "args": more, "loci": heads, "annotation": anno, "annotation_gff3": anno3, "report": report_block(out),
                               "predicted": predicted_transcripts(outu), "reader_stderr": err}
        print(key, heads)
        print(report_block(out))
    with gzip.GzipFile(os.path.join(HERE, "golden_genbank.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(gold, indent=0, sort_keys=True).encode())


if __name__ == "__main__":
    main()
