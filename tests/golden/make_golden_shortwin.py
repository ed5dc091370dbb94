#!/usr/bin/env python3
"""Goldens from the REAL reference (oracle/_ref, built by oracle/Makefile) for the species whose translation-initiation window is
shorter than a block of the dense kernels: Micromonas_pusilla, Rhopilema_esculentum, galdieria (--UTR=off) and schistosoma
(tests/shortwin_cases.py: SHORTWIN_CFGS; their parameter files are config_shortwin.tar.gz, the species directories of the reference's
configuration tree without the splice-site files that only its training reads).  Run where oracle/_ref exists:
    python tests/golden/make_golden_shortwin.py

Outputs, per configuration <cfg>:
  golden_shortwin_<cfg>.gff          the reference binary's prediction on shortwin_records(cfg) at the species' defaults (sample = 100)
  golden_shortwin_<cfg>_<variant>.gff  the same with the options of shortwin_cases.VARIANTS: pieces (--maxDNAPieceSize=9000: the records
                                     with the start codon / donor site motifs are cut in at least two places), softmasking (on records with
                                     a lower-case third), single (--singlestrand=true), complete (--genemodel=complete)
  golden_shortwin_paths_<cfg>.json   ln Viterbi and the Viterbi state path [(begin, end, type)] of every record (oracle/_ref/ref_harness),
                                     and how many INITIAL states of the path begin in the block of 8, 4 and 2 bases they end in
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from helpers import REF_AUGUSTUS, gff_body, ref_harness, write_fasta  # noqa
from shortwin_cases import INITIAL_TYPES, SHORTWIN_CFGS, VARIANTS, ref_args, shortwin_config_path, shortwin_records, variant_records  # noqa


def main():
    d = tempfile.mkdtemp()
    env = dict(os.environ, AUGUSTUS_CONFIG_PATH=shortwin_config_path())
    for cfg, (species, opts) in SHORTWIN_CFGS.items():
        if cfg == "galdieria_utr":  # (refused for its UTR windows: no golden)
            continue
        recs = shortwin_records(cfg)
        for variant in [None] + list(VARIANTS):
            fa = os.path.join(d, "%s_%s.fa" % (cfg, variant))
            write_fasta(fa, variant_records(cfg, variant))
            r = subprocess.run([REF_AUGUSTUS] + ref_args(cfg, variant) + [fa], capture_output=True, text=True, env=env)
            assert r.returncode == 0, r.stderr[-2000:]
            body = gff_body(r.stdout)
            open(os.path.join(HERE, "golden_shortwin_%s%s.gff" % (cfg, "_" + variant if variant else "")), "w").write("\n".join(body) + "\n")
            print(cfg, variant or "defaults", len(body), "lines,", sum("\tgene\t" in l for l in body), "genes")
        fa = os.path.join(d, cfg + "_None.fa")
        res, err = ref_harness(fa, species, ["--%s=%s" % kv for kv in opts.items()], cfg=shortwin_config_path())
        assert len(res) == len(recs), err[-2000:]
        out = []
        for (name, seq), r in zip(recs, res):
            short = {str(b): sum(1 for bg, en, t in r["path"] if t in INITIAL_TYPES and bg - 1 >= (en // b) * b) for b in (8, 4, 2)}
            out.append({"name": name, "len": len(seq), "lnv": repr(r["lnv"]), "path": r["path"], "initial_in_block": short})
            print(" ", name, len(seq), "elements", len(r["path"]), "initial states that begin in their own block (8 / 4 / 2):", short)
        json.dump({"records": out}, open(os.path.join(HERE, "golden_shortwin_paths_%s.json" % cfg), "w"), indent=0)


if __name__ == "__main__":
    main()
