"""The four species whose translation-initiation window is shorter than the smallest block of the dense kernels (Micromonas_pusilla,
Rhopilema_esculentum, galdieria, schistosoma): configuration tree, model options and the records made for them.  Their INITIAL
candidates are in the late class of the dense kernels (dp.h: isLateKind); shared by tests/test_shortwin_cpu.py and
tests/test_shortwin_gpu.py and by tests/golden/make_golden_shortwin.py."""
import os
import random
import shutil
import tarfile
import tempfile

from helpers import GOLDEN, config_path, golden_inputs, random_dna

# cfg -> (species, options).  Each species at its own defaults (sample = 100 everywhere; galdieria: UTR = on, 71 states); galdieria
# without its UTR states is the fifth configuration
SHORTWIN_CFGS = {
    "micromonas": ("Micromonas_pusilla", {}),
    "rhopilema": ("Rhopilema_esculentum", {}),
    "galdieria": ("galdieria", {"UTR": "off"}),
    "galdieria_utr": ("galdieria", {}),
    "schistosoma": ("schistosoma", {}),
}
# trans_init_window and dss_start of the species (their *_parameters.cfg): the shortest initial exon state is
# min(W, W + minexonlength - dss_start) bases long, clamped to 1 by the reference
WINDOWS = {"micromonas": (3, 3), "rhopilema": (3, 3), "galdieria": (0, 1), "galdieria_utr": (0, 1), "schistosoma": (0, 3)}
K_INITIAL = 2  # include/augx.h: AUGX_K_INITIAL
INITIAL_TYPES = (2, 3, 4)  # state types initial0..2 (the reference's StateType)

_cfg_dir = None


def shortwin_config_path():
    """the configuration tree of helpers.config_path() with the four species of config_shortwin.tar.gz next to the others, in a temporary
    directory of its own (the shared tree is linked, not copied, and not written to)"""
    global _cfg_dir
    if _cfg_dir is None:
        tar = os.path.join(GOLDEN, "config_shortwin.tar.gz")
        base = config_path()
        d = os.path.join(tempfile.gettempdir(), "augx_shortwin_%d_%d_%s" % (os.getuid(), os.path.getsize(tar), os.path.basename(os.path.dirname(os.path.dirname(base)))))
        marker = os.path.join(d, "config", "species", "schistosoma", "schistosoma_parameters.cfg")
        if not os.path.exists(marker):
            tmp = tempfile.mkdtemp(prefix="augx_shortwin_tmp_")
            os.makedirs(os.path.join(tmp, "config", "species"))
            for e in os.listdir(base):
                if e != "species":
                    os.symlink(os.path.join(base, e), os.path.join(tmp, "config", e))
            for e in os.listdir(os.path.join(base, "species")):
                os.symlink(os.path.join(base, "species", e), os.path.join(tmp, "config", "species", e))
            with tarfile.open(tar) as t:
                t.extractall(tmp)
            try:
                os.rename(tmp, d)
            except OSError:
                if os.path.exists(marker):
                    shutil.rmtree(tmp, ignore_errors=True)
                else:
                    d = tmp
        _cfg_dir = os.path.join(d, "config") + "/"
    return _cfg_dir


def shortwin_model(cfg):
    import augustus_amd as ax
    species, opts = SHORTWIN_CFGS[cfg]
    return ax.Model(shortwin_config_path(), species, **opts)


# ---------------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------------
_CODONS = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT" if a + b + c not in ("TAA", "TAG", "TGA")]


def _orf(rng, codons, gc=0.5):
    """codons without a stop in any phase-0 reading: an open reading frame"""
    pool = [c for c in _CODONS if "TA" not in c and "TG" not in c[:2]]  # (no stop across codon borders in the other frames either)
    w = [1.0 + (gc - 0.5) * 2 * (sum(ch in "GC" for ch in c) - 1.5) for c in pool]
    return "".join(rng.choices(pool, weights=w, k=codons))


def start_donor_motif(coding, rng, gc=0.5):
    """a start codon followed by a donor site after `coding` coding bases (the start codon included): an initial exon of that
    length; then a short intron, and an open reading frame in the phase the exon leaves, down to a stop codon"""
    body = _orf(rng, (coding + 2) // 3 + 1, gc)[:coding - 3]
    intron = "GTAAGT" + "".join(rng.choice("ACT") for _ in range(58)) + "TTTTCTTTTTCTCTTTCAG"
    rest = _orf(rng, 70, gc)
    phase = coding % 3  # bases of the split codon already in the first exon
    tail = rest[phase:] if phase else rest
    return "GCCGCCACC" + "ATG" + body + intron + tail + "TAA"


def motif_record(cfg, seed, lead=0, gc=0.5, copies=None):
    """(a) start codons followed by a donor site after 3, 4, ... W + 8 + 2 coding bases, one copy of each length at every offset of a
    block of 8 (and so of 4 and of 2): spacers of random DNA whose length steps by one put the end of the initial exon state on
    every lane position.  lead: bases of random DNA before the first motif"""
    W, _ = WINDOWS[cfg]
    rng = random.Random(seed)
    bg = lambda n: "".join(rng.choice("GC") if rng.random() < gc else rng.choice("AT") for _ in range(n))
    parts = [bg(lead)]
    lens = list(range(3, W + 8 + 2 + 1))
    for k in range(copies or 8):
        for L in lens:
            parts.append(start_donor_motif(L, rng, gc))
            parts.append(bg(120 + (k + L) % 8))
    return "".join(parts)


def edge_record(cfg, seed):
    """(b) the motif in the first block and in the last block of a piece: the record begins with a start codon at base 0 .. 7 and
    ends a few bases after a donor site (a right-truncated initial exon; with UTR states the last block is made twice, redoBlock)"""
    rng = random.Random(seed)
    W, _ = WINDOWS[cfg]
    head = "".join(start_donor_motif(3 + k, rng)[9 - min(9, k):] + random_dna(150 + k, seed + k) for k in range(W + 6))
    tail = "GCCGCCACCATGG" + _orf(rng, 2)[:4 + W] + "GTAAGT"[:rng.randint(0, 6)]
    return head + random_dna(700, seed + 99) + tail


def gc_step_record(seed):
    """(c) the motifs across steps of GC class (schistosoma has five): stretches of 30 %, 45 % and 60 % GC (three classes), motifs of the matching
    composition right at the steps and inside"""
    rec = []
    for i, gc in enumerate((0.30, 0.45, 0.60)):
        rec.append(motif_record("schistosoma", seed + i, lead=2500, gc=gc, copies=2))
    return "".join(rec)


PIECE = 9000  # --maxDNAPieceSize of the runs that cut the records (the motif records are 21-29 kb: at least two cuts)


# runs of the executable beside the species' defaults: golden_shortwin_<cfg>_<variant>.gff
VARIANTS = {
    "pieces": {"maxDNAPieceSize": str(PIECE)},   # the cut finder's exam windows; cuts through the records with the motifs
    "softmasking": {"softmasking": "1"},         # on records with a lower-case third
    "single": {"singlestrand": "true"},          # the 24-state model, every record as it is and reverse-complemented
    "complete": {"genemodel": "complete"},
}


def ref_args(cfg, variant=None):
    """command line of the reference binary / the executable for one configuration (the input file is appended)"""
    species, opts = SHORTWIN_CFGS[cfg]
    opts = {**opts, **(VARIANTS[variant] if variant else {})}
    return ["--species=" + species] + ["--%s=%s" % kv for kv in opts.items()]


def revcomp_records(recs):
    comp = str.maketrans("ACGTacgt", "TGCAtgca")
    return [(n + "_rc", s[::-1].translate(comp)) for n, s in recs]


def variant_records(cfg, variant=None):
    recs = shortwin_records(cfg)
    if variant == "softmasking":  # (the bonus of lower-case bases on the intergenic and intron states)
        recs = [(n, s[:len(s) // 3] + s[len(s) // 3:2 * len(s) // 3].lower() + s[2 * len(s) // 3:]) for n, s in recs]
    return recs


def shortwin_records(cfg):
    """[(name, sequence)] of 2-30 kb for one configuration"""
    recs = [("motifs", motif_record(cfg, 7100, copies=6)), ("edges", edge_record(cfg, 7200))]
    if cfg == "schistosoma":
        recs.append(("gcsteps", gc_step_record(7300)))
        # (found by a search over seeds: the reference itself predicts an initial exon here whose state is three bases long and
        #  begins in the block of eight it ends in)
        recs.append(("motifs_path", motif_record(cfg, 105, copies=2)))
    recs.append(("HS04636", dict(golden_inputs())["HS04636"]))
    recs.append(("rand20k", random_dna(20000, 7400)))
    return recs


def in_block_initials(path, kinds, blk):
    """elements of a state path [(begin, end, state, type)] that are INITIAL states whose predecessor ends in the block of their own
    end: begin - 1 >= (end // blk) * blk"""
    return [(b, e, s) for b, e, s, _ in path if kinds[s] == K_INITIAL and b - 1 >= (e // blk) * blk]
