#!/usr/bin/env python3
"""Golden vectors of heated posterior sampling (--temperature=3) from the REAL reference (oracle/_ref), with the configuration
of tests/golden/config_*.tar.gz.  Run where the reference has been built:
    python tests/golden/make_golden_heated.py [cfg ...]      (no argument: every configuration of HEATED_CFGS)

  golden_heated_<cfg>.gff          the reference binary's GFF (prediction part) of helpers.SAMPLED_CFGS[cfg] run with
                                   --temperature=3 added (the number of samples is the configuration's: the species' default of 100, 50 for human1_sm, 30 for human_utr_alt)
  golden_heated_<cfg>.head         the header line the reference prints for the option ("# setting temperature to 3 (for sampling)")
  golden_heated_paths_<cfg>.json   per record the first 5 sampled state paths of ref_harness --dumpsamples under --temperature=3
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from helpers import *  # noqa

# fly (47 states), human with the soft-masking bonus (47 states), human with UTR states (71 states, dense kernels)
HEATED_CFGS = ("fly", "fly_alt", "human1_sm", "human_utr_alt")
TEMPERATURE = "3"


def heated_options(cfg):
    species, opts, _ = SAMPLED_CFGS[cfg]
    return species, dict(opts, temperature=TEMPERATURE)


def main():
    env = dict(os.environ, AUGUSTUS_CONFIG_PATH=config_path())
    d = tempfile.mkdtemp()
    for cfg in HEATED_CFGS:
        if len(sys.argv) > 1 and cfg not in sys.argv[1:]:
            continue
        species, opts = heated_options(cfg)
        recs = sampled_records(cfg)
        fa = os.path.join(d, cfg + ".fa")
        write_fasta(fa, recs)
        extra = ["--%s=%s" % kv for kv in opts.items()]
        txt = subprocess.run([REF_AUGUSTUS, "--species=" + species] + extra + [fa], capture_output=True, text=True, env=env)
        assert txt.returncode == 0 and txt.stderr == "", txt.stderr
        body = gff_body(txt.stdout)
        head = [l for l in txt.stdout.splitlines() if l.startswith("# setting temperature")]
        assert head == ["# setting temperature to %s (for sampling)" % TEMPERATURE], head
        open(os.path.join(HERE, "golden_heated_%s.gff" % cfg), "w").write("\n".join(body) + "\n")
        open(os.path.join(HERE, "golden_heated_%s.head" % cfg), "w").write("\n".join(head) + "\n")
        if cfg != "fly_alt":  # (the sampled paths do not depend on what the gene stage makes of them: fly's are fly_alt's)
            smp = ref_samples(fa, species, extra, 5)
            json.dump({"species": species, "records": [{"name": n, "samples": s} for (n, _), s in zip(recs, smp)]},
                      open(os.path.join(HERE, "golden_heated_paths_%s.json" % cfg), "w"))
        print(cfg, len(recs), "records", len(body), "gff lines")


if __name__ == "__main__":
    main()
