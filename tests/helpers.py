"""Shared test plumbing: config fixture, oracle (twin / reference harness) wrappers, FASTA I/O.

The oracle libraries (oracle/libghmm_twin.so, oracle/_ref/*) are loaded ONLY from here, i.e. from tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg -- never from augustus_amd/.
"""
import ctypes
import os
import random
import subprocess
import tarfile
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TWIN_LIB = os.path.join(ROOT, "oracle", "libghmm_twin.so")
REF_HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
REF_AUGUSTUS = os.path.join(ROOT, "oracle", "_ref", "augustus_ref")
EMU_LIB = os.environ.get("AUGX_EMU_LIB") or os.path.join(ROOT, "build", "libaugx_emu.so")  # (AUGX_EMU_LIB: the emulator built with other build-time switches)

# tests that compare with the REAL reference (oracle/_ref, built by oracle/Makefile where /root/reference exists; the binaries
# travel to the GPU box with the working tree).  Without them such a test is skipped on the CPU -- and FAILS in the GPU suite or
# with AUGX_REQUIRE_REF=1 (tests/conftest.py): a parity run must not go green because its checker was missing.
import pytest
needs_ref = pytest.mark.needs_ref

_cfg_dir = None


def config_path():
    """AUGUSTUS_CONFIG_PATH-style directory: extracted from the committed fixture (works on the GPU box)."""
    global _cfg_dir
    if _cfg_dir is None:
        tar = os.path.join(GOLDEN, "config_min.tar.gz")
        more = os.path.join(GOLDEN, "config_more.tar.gz")  # two more species (nasonia: 5 GC classes, rice: 4)
        caeno = os.path.join(GOLDEN, "config_caeno.tar.gz")  # caenorhabditis (the reference's own test_ab_initio_prediction); Vitrella_brassicaformis, maize (47-state models the dense kernels take), chlamy2011 (gc donor sites, UTR tables of order 3), tetrahymena (translation table 6, intron content of order 3)
        d = os.path.join(tempfile.gettempdir(), "augx_config_%d_%d_%d_%d" % (os.getuid(), os.path.getsize(tar), os.path.getsize(more), os.path.getsize(caeno)))
        marker = os.path.join(d, "config", "model", "states_shadow.cfg")
        if not os.path.exists(marker):
            # several processes may get here at once (one rank per GPU, pytest-xdist): extract privately, publish with one
            # atomic rename; whoever loses the race uses the winner's copy
            import shutil
            tmp = tempfile.mkdtemp(prefix="augx_config_tmp_")
            for tf in (tar, more, caeno):
                with tarfile.open(tf) as t:
                    t.extractall(tmp)
            try:
                os.rename(tmp, d)
            except OSError:
                if os.path.exists(marker):
                    shutil.rmtree(tmp, ignore_errors=True)
                else:
                    d = tmp  # (a stale, incomplete directory is in the way: use the private copy)
        _cfg_dir = os.path.join(d, "config") + "/"
    return _cfg_dir


def read_fasta(fn):
    recs, name, seq = [], None, []
    for line in open(fn):
        line = line.strip()
        if line.startswith(">"):
            if name is not None:
                recs.append((name, "".join(seq)))
            name, seq = line[1:].split()[0], []
        else:
            seq.append("".join(ch for ch in line if ch.isalpha()))
    if name is not None:
        recs.append((name, "".join(seq)))
    return recs


def write_fasta(fn, recs, width=60):
    with open(fn, "w") as f:
        for name, s in recs:
            f.write(">%s\n" % name)
            for k in range(0, len(s), width):
                f.write(s[k:k + width] + "\n")


def random_dna(n, seed, alphabet="ACGT"):
    rng = random.Random(seed)
    return "".join(rng.choice(alphabet) for _ in range(n))


class _St(ctypes.Structure):
    _fields_ = [("begin", ctypes.c_int32), ("end", ctypes.c_int32), ("state", ctypes.c_int16), ("type", ctypes.c_int16)]


_twin = None


def twin():
    global _twin
    if _twin is None:
        _twin = ctypes.CDLL(TWIN_LIB)
    return _twin


def twin_tss0_carry(on):
    """consecutive twin_decode calls are the reference's consecutive sequences: entry 0 of its TSS caches lives on while they keep one
    length (oracle/ghmm_twin.cc: twin_set_tss0_carry); off: every call starts with empty caches"""
    twin().twin_set_tss0_carry(1 if on else 0)


def twin_decode(tables_ptr, seq, S, cells=False, init_kind=0, term_kind=0, cache=None):
    """CPU oracle (oracle/ghmm_twin.cc).  Returns (status, lnv, [(begin,end,state,type)], V or None, gc).
    cache: the restated SnippetProbs cache of the reference (multi-class pieces) on or off; by default it follows
    AUGX_EXACT_MULTICLASS like the emulator, so that a test that switches the device's exact mode off compares like with like."""
    n = len(seq)
    if cache is None:
        cache = os.environ.get("AUGX_EXACT_MULTICLASS", "1") != "0"
    twin().twin_set_snippet_cache(1 if cache else 0)
    V = np.empty((n, S)) if cells else None
    gc = np.empty(n, dtype=np.int32)
    cap = max(1024, n // 4 + 16)
    sts = (_St * cap)()
    ns, lnv = ctypes.c_int32(), ctypes.c_double()
    rc = twin().twin_decode(tables_ptr, seq.encode() if isinstance(seq, str) else seq, ctypes.c_int64(n), init_kind, term_kind,
                            V.ctypes.data_as(ctypes.c_void_p) if cells else None, gc.ctypes.data_as(ctypes.c_void_p),
                            sts, cap, ctypes.byref(ns), ctypes.byref(lnv))
    path = [(sts[i].begin, sts[i].end, sts[i].state, sts[i].type) for i in range(ns.value)]
    return rc, lnv.value, path, V, gc


def twin_chain_states(tables_ptr, S):
    """the reachable single-base chain states of the model in the order of the state index: byte c of a bpChain record is state [c]"""
    out = np.zeros(S, dtype=np.int32)
    k = twin().twin_chain_states(tables_ptr, out.ctypes.data_as(ctypes.c_void_p))
    return [int(x) for x in out[:k]]


def twin_tie_classes(tables_ptr, S):
    """(class, kind) of every state: class 0 not reachable, 1 single-base chain state, 2 variable-length state (exon kinds, lessD, UTR exon
    kinds: its elements on a path can be counted as near ties), 3 fixed-lag state (never counted); kind: AUGX_K_*"""
    c, k = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
    twin().twin_tie_classes(tables_ptr, c.ctypes.data_as(ctypes.c_void_p), k.ctypes.data_as(ctypes.c_void_p))
    return [int(x) for x in c], [int(x) for x in k]


class TwinTies:
    """what oracle/ghmm_twin.cc: twin_near_ties says about one piece (the definition of DESIGN.md 6, "near-ties"):
    rc, lnv, path, V as twin_decode; margin / margin_full [n, S]: winner - runner-up of every live chain cell under the rule of the kernel
    family / the full definition (+inf: no runner-up, NaN: not a live chain cell); items: [(base, state, rule, margin, margin_full)], what the
    count of the piece is made of, 3' to 5' (rule 0: entry cell of a chain run, 1: another cell of it, 2: variable-length element)"""

    def __init__(self, tables_ptr, seq, S, family, init_kind=0, term_kind=0, cache=None):
        n = len(seq)
        if cache is None:
            cache = os.environ.get("AUGX_EXACT_MULTICLASS", "1") != "0"
        twin().twin_set_snippet_cache(1 if cache else 0)
        self.n, self.S, self.family = n, S, family
        self.all_n = not any(c in "ACGTacgt" for c in (seq if isinstance(seq, str) else seq.decode()))  # (a piece without a nucleotide)
        self.V, self.margin, self.margin_full = np.empty((n, S)), np.empty((n, S)), np.empty((n, S))
        cap, pcap = n + 16, max(1024, n // 4 + 16)
        lst, lm = np.zeros((cap, 7), dtype=np.int32), np.zeros((cap, 2))
        sts = (_St * pcap)()
        nl, c, cf, ns, lnv = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_double()
        T = twin()
        T.twin_near_ties.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double] + \
                                    [ctypes.c_void_p] * 4 + [ctypes.c_int64] + [ctypes.POINTER(ctypes.c_int64)] * 3 + \
                                    [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)]
        self.rc = T.twin_near_ties(tables_ptr, seq.encode() if isinstance(seq, str) else seq, n, init_kind, term_kind, family, 1.0,
                                   self.margin.ctypes.data_as(ctypes.c_void_p), self.margin_full.ctypes.data_as(ctypes.c_void_p),
                                   lst.ctypes.data_as(ctypes.c_void_p), lm.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(nl), ctypes.byref(c), ctypes.byref(cf),
                                   self.V.ctypes.data_as(ctypes.c_void_p), sts, pcap, ctypes.byref(ns), ctypes.byref(lnv))
        assert nl.value <= cap and ns.value <= pcap
        self.lnv = lnv.value
        self.path = [(sts[i].begin, sts[i].end, sts[i].state, sts[i].type) for i in range(ns.value)]
        self.items = [(int(lst[i, 0]), int(lst[i, 1]), int(lst[i, 2]), float(lm[i, 0]), float(lm[i, 1])) for i in range(nl.value)]
        # (base, state) of a variable-length element -> (live candidates of its cell, the runner-up shares the winner's predecessor end and differs in the ancestor,
        # some two live candidates of the cell share a predecessor end, exon length of the runner-up, of the winner -- coding exons, else 0)
        self.cands = {(int(lst[i, 0]), int(lst[i, 1])): (int(lst[i, 3]), bool(lst[i, 4] & 1), bool(lst[i, 4] & 2), int(lst[i, 5]), int(lst[i, 6])) for i in range(nl.value) if lst[i, 2] == 2}
        assert self.counts(1.0) == (c.value, cf.value)  # (the twin's own sums at the threshold it was called with)

    def counts(self, eps):
        """(count, count under the full definition) of the piece at threshold eps: the flagged chain cells of the path's chain runs and
        the variable-length elements of the path with 0 < margin < eps (an exact tie of a variable-length element is not counted)"""
        c = sum(1 for _, _, rule, mk, _ in self.items if mk < eps and (rule < 2 or mk != 0.0))
        cf = sum(1 for _, _, rule, _, mf in self.items if mf < eps and (rule < 2 or mf != 0.0))
        return c, cf

    def flags(self, eps, full=False):
        """[n, S] int8: -1 not a live chain cell, 1 flagged at threshold eps, 0 not"""
        m = self.margin_full if full else self.margin
        with np.errstate(invalid="ignore"):
            return np.where(np.isnan(m), -1, (m < eps).astype(np.int8)).astype(np.int8)


def chain_flags_of(bytes_, chain_states, S, dense=False):
    """the near-tie flags a decode left (Batch.prep / emu_prep, "bpChain" [n, 8] or "bpD" [n * S]) in the shape of TwinTies.flags: [n, S]
    int8, -1: no value (base 0 of a piece holds none), -2: the dense kernels' mark of a piece of N only"""
    if dense:
        b = np.asarray(bytes_).reshape(-1, S)
        out = np.full(b.shape, -1, dtype=np.int8)
        for s in chain_states:
            out[:, s] = np.where(b[:, s] == 0xFF, -1, np.where(b[:, s] == 0xFE, -2, (b[:, s] >> 6) & 1))  # (0xFE: a piece of N only)
    else:
        b = np.asarray(bytes_).reshape(-1, 8)
        out = np.full((len(b), S), -1, dtype=np.int8)
        for c, s in enumerate(chain_states):
            out[:, s] = np.where(b[:, c] == 0xFF, -1, b[:, c] >> 7)
    out[0, :] = -1
    return out


class BumpedTables:
    """the tables of model m with entry `length` of the length distribution of the coding exons of kind `kind` raised by delta (oracle/
    ghmm_twin.cc: twin_tables_bump_exon_length; everything else is shared with m, which it keeps alive): stands in for a model where twin
    and emulator take one (tables_ptr, n_states)"""

    def __init__(self, m, kind, length, delta):
        T = twin()
        T.twin_tables_bump_exon_length.restype = ctypes.c_void_p
        T.twin_tables_bump_exon_length.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double]
        T.twin_tables_free.argtypes = [ctypes.c_void_p]
        self.model, self.n_states = m, m.n_states
        self._p = T.twin_tables_bump_exon_length(m.tables_ptr, kind, length, delta)
        assert self._p

    @property
    def tables_ptr(self):
        return ctypes.c_void_p(self._p)

    def __del__(self):
        if getattr(self, "_p", None):
            twin().twin_tables_free(self._p)
            self._p = None


def emu_set_near_tie_eps(eps, lib=None):
    """the threshold of the near-tie counter for the emulator's decodes from now on (tests/emu/emu.cc; None: the product's)"""
    E = _emu_of(lib)
    E.emu_set_near_tie_eps.argtypes = [ctypes.c_double]
    return E.emu_set_near_tie_eps(2e-7 if eps is None else float(eps))


def emu_near_ties(n, lib=None):
    """near ties the emulator's back-trace counted on the paths of the n pieces of its last decode"""
    E = _emu_of(lib)
    return [E.emu_near_ties(i) for i in range(n)]


def twin_cache_log(tables_ptr, seq, S, cells=False, init_kind=0, term_kind=0):
    """twin_decode with the restated caches on and their log kept (oracle/ghmm_twin.cc: twin_set_cache_log).  Returns
    (twin_decode's tuple, {(j, s, eop): term} of every short-intron request the SnippetProbs cache answered with another content than
    the class of j gives, [(q, asking column, asking state, class)] of every computation of a forward acceptor-site value into the
    aSSProb memo in the order of the calls, the number of times the memo was emptied)."""
    T = twin()
    T.twin_snippet_log.restype = T.twin_site_log.restype = ctypes.c_int64
    T.twin_memo_flushes.restype = ctypes.c_longlong
    T.twin_set_cache_log(1)
    try:
        res = twin_decode(tables_ptr, seq, S, cells=cells, init_kind=init_kind, term_kind=term_kind, cache=True)
        n = T.twin_snippet_log(None, None, ctypes.c_int64(0))
        keys, te = np.zeros((max(n, 1), 3), dtype=np.int32), np.zeros(max(n, 1))
        T.twin_snippet_log(keys.ctypes.data_as(ctypes.c_void_p), te.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(n))
        terms = {}
        for k, v in zip(keys[:n].tolist(), te[:n].tolist()):
            assert tuple(k) not in terms, k  # (a request is made once)
            terms[tuple(k)] = v
        m = T.twin_site_log(None, ctypes.c_int64(0))
        sites = np.zeros((max(m, 1), 4), dtype=np.int32)
        T.twin_site_log(sites.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(m))
        return res, terms, [tuple(r) for r in sites[:m].tolist()], int(T.twin_memo_flushes())
    finally:
        T.twin_set_cache_log(0)


def site_changes(sites):
    """the log of site computations -> [(q, key, class)] as the replay keeps its history (assmemo.h: hist): a computation that gives a
    site the class it had before changes no value and is left out; key = (column << 7) | state"""
    last, out = {}, []
    for q, j, s, c in sites:
        if last.get(q) != c:
            last[q] = c
            out.append((q, (j << 7) | s, c))
    return out


def ref_harness(fasta, species, extra=(), cells_file=None, cfg=None):
    """The REAL reference through oracle/_ref/ref_harness.  Returns list of dicts per record."""
    env = dict(os.environ, AUGUSTUS_CONFIG_PATH=cfg or config_path())
    cmd = [REF_HARNESS, "--species=" + species] + list(extra)
    if cells_file:
        cmd.append("--dumpcells=" + cells_file)
    cmd.append(fasta)
    out = subprocess.run(cmd, capture_output=True, text=True, env=env)
    res, cur = [], None
    for line in out.stdout.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "SEQ":
            cur = {"name": w[1], "n": int(w[2]), "path": [], "lnv": None}
        elif w[0] == "LNV":
            cur["lnv"] = float(w[1])
        elif w[0] == "ST":
            cur["path"].append((int(w[1]), int(w[2]), int(w[3])))
        elif w[0] == "ERR":
            cur["err"] = line
        elif w[0] == "END":
            res.append(cur)
    return res, out.stderr


def ref_forward(fasta, species, extra=(), cfg=None):
    """ln of the REAL reference's forward variables (oracle/_ref/ref_harness --sample=100 --dumpforward): one [len, S] array
    per record, -inf where the cell is absent"""
    import struct
    dump = fasta + ".fwd.bin"
    env = dict(os.environ, AUGUSTUS_CONFIG_PATH=cfg or config_path())
    out = subprocess.run([REF_HARNESS, "--species=" + species, "--sample=100"] + list(extra) + ["--dumpforward=" + dump, fasta],
                         capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    mats = []
    with open(dump, "rb") as f:
        while True:
            h = f.read(8)
            if len(h) < 8:
                break
            n, S = struct.unpack("ii", h)
            mats.append(np.frombuffer(f.read(n * S * 8), dtype=np.float64).reshape(n, S))
    os.remove(dump)
    return mats


def ref_samples(fasta, species, extra=(), n=5, cfg=None):
    """n sampled state paths per record from the REAL reference (oracle/_ref/ref_harness --dumpsamples: NAMGene::getSampledPath,
    rand() never seeded): [[(begin, end, type), ...] per sample] per record"""
    dump = fasta + ".smp.txt"
    env = dict(os.environ, AUGUSTUS_CONFIG_PATH=cfg or config_path())
    ex = [e for e in extra if not e.startswith("--sample=")]
    out = subprocess.run([REF_HARNESS, "--species=" + species, "--sample=100"] + ex + ["--dumpsamples=" + dump, "--nsamples=%d" % n, fasta],
                         capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    recs = []
    for l in open(dump):
        w = l.split()
        if w[0] == "SEQ":
            recs.append([])
        elif w[0] == "SAMPLE":
            recs[-1].append([])
        else:
            recs[-1][-1].append([int(x) for x in w[1:4]])
    os.remove(dump)
    return recs


# ---------------------------------------------------------------------------------------------------
# golden vectors (tests/golden/make_golden.py) and the lane-loop emulator of the device kernels
# ---------------------------------------------------------------------------------------------------
import json

GOLDEN_CFGS = {
    "human": ("human", {}),
    "human_nosm": ("human", {"softmasking": "0"}),
    "fly": ("fly", {"UTR": "off", "sample": "0", "softmasking": "0"}),
    "arabidopsis": ("arabidopsis", {"UTR": "off", "sample": "0", "softmasking": "0"}),
    "saccharomyces": ("saccharomyces", {"UTR": "off", "sample": "0", "softmasking": "0"}),
    "human_intronless": ("human", {"genemodel": "intronless", "softmasking": "0"}),          # 3 states; several GC classes in a piece
    "fly_intronless": ("fly", {"genemodel": "intronless", "UTR": "off", "sample": "0"}),     # with the soft-masking bonus
    # --UTR=on: the 71-state model with untranslated regions (dense kernels, device/dense.h)
    "human_utr": ("human", {"UTR": "on"}),
    "human_utr_nosm": ("human", {"UTR": "on", "softmasking": "0"}),
    "fly_utr": ("fly", {"sample": "0"}),                                                    # UTR on is the species' default
    "fly_utr_print": ("fly", {"sample": "0", "softmasking": "0", "print_utr": "on", "gff3": "on", "introns": "on"}),
}


# species pinned at a larger scale (tests/golden/make_golden_big.py: more_species): 300 kb of real DNA and records whose GC
# content runs through many classes, at the species' own maxDNAPieceSize (200 kb: one cut)
MORE_CFGS = {
    "nasonia": ("nasonia", {"UTR": "off", "sample": "0", "softmasking": "0"}),
    "rice": ("rice", {"UTR": "off", "sample": "0", "softmasking": "0"}),
    # two fungi whose equalD states look back 64 and 112 bases (dStateLen = d - splice windows): one to two tiles -- their predecessors
    # may lie in the tile before the current one, which is not in HBM yet when the current tile's long-lag values are staged
    "fusarium_graminearum": ("fusarium_graminearum", {"UTR": "off", "softmasking": "0"}),          # dStateLen 64; sample = 100 (default)
    "phanerochaete_chrysosporium": ("phanerochaete_chrysosporium", {"UTR": "off", "sample": "0", "softmasking": "0"}),  # 112
}


# gene models with two intergenic states (--genemodel=atleastone / exactlyone: states_shadow_2igenic.cfg, the synch state is the
# second intergenic state; dense kernels).  Records in which such a model has no feasible path (no room for a gene) are left out:
# the reference ends the whole run with an error there (tests/test_cli_errors.py)
GENEMODEL_CFGS = {
    "human_atleastone": ("human", {"genemodel": "atleastone"}),                                   # soft-masking bonus on
    "fly_exactlyone": ("fly", {"genemodel": "exactlyone", "UTR": "off", "softmasking": "0"}),    # sample = 100 (the species' default)
}


def gc_step_records(count, seed, parts=8, lo=2500, hi=6000):
    """records of uniform-random stretches whose GC content steps every few kb (two to five GC classes under most models): what the
    reference's call-history caches (SnippetProbs, tssProbsPlus, the aSSProb memo) are sensitive to"""
    rng = random.Random(seed)
    recs = []
    for i in range(count):
        p = []
        for k in range(parts):
            gc = rng.choice([0.35, 0.42, 0.5, 0.58, 0.65])
            p.append("".join(rng.choice("GC") if rng.random() < gc else rng.choice("AT") for _ in range(rng.randint(lo, hi))))
        recs.append(("gcsteps%d_%d" % (seed, i), "".join(p)))
    return recs


def n_window_record(seed=5, gcs=(0.36, 0.62), run=12000):
    """a stretch of low GC content, a run of N longer than the GC window (GCwinsize 10000), a stretch of high GC content: inside the run
    there are windows without a single nucleotide -- the reference classes them by the composition of the FIRST window of the piece
    (BaseCount::normalize leaves the relative frequencies alone when the counts sum to 0, src/motif.cc:204-212,561-575)"""
    rng = random.Random(seed)
    part = lambda n, gc: "".join(rng.choice("GC") if rng.random() < gc else rng.choice("AT") for _ in range(n))
    return ("nwin%d" % seed, part(26000, gcs[0]) + "N" * run + part(24000, gcs[1]))


def genemodel_records():
    return [(n, s) for n, s in golden_inputs() if n not in ("allN", "short7", "short100")]


def more_inputs():
    return read_fasta(os.path.join(GOLDEN, "inputs_more.fa"))


# posterior sampling (tests/golden/make_golden_sampled.py): cfg -> (species, options, record names of inputs.fa or None = all).
# (human1: the records with one GC class; human_all: every record)
_ONE_CLASS = ("HS04636", "HS08198", "rand20k_b", "withN", "allN", "short7", "short100", "short600", "iupac", "trunc_left", "trunc_right",
              "trunc_both", "revcomp", "softmask_rand")
SAMPLED_CFGS = {
    "fly": ("fly", {"UTR": "off", "softmasking": "0"}, None),                 # sample = 100 is the species' default
    "fly_sm": ("fly", {"UTR": "off"}, None),
    "arabidopsis": ("arabidopsis", {"UTR": "off", "softmasking": "0", "sample": "100"}, None),
    "human1": ("human", {"sample": "100", "softmasking": "0"}, _ONE_CLASS),
    "human1_sm": ("human", {"sample": "50"}, _ONE_CLASS),
    # the probability filter (src/gene.cc:2489-2512) with the Viterbi transcripts not exempt: genes drop out, the numbering follows
    # all records incl. the ones with several GC classes in a piece (the reference's snippet cache around the class steps is replayed)
    "human_all": ("human", {"sample": "100", "softmasking": "0"}, None),
    "fly_filter": ("fly", {"UTR": "off", "softmasking": "0", "keep_viterbi": "false", "minexonintronprob": "0.3", "minmeanexonintronprob": "0.6"}, None),
    # --alternatives-from-sampling=true: the sampled transcripts that pass the filter stay, overlapping ones of one strand and reading
    # frame become the alternatives t1, t2, ... of a gene (sorted by mean state probability); --maxtracks bounds how many may overlap
    "fly_alt": ("fly", {"UTR": "off", "softmasking": "0", "alternatives-from-sampling": "true"}, None),
    "human_alt": ("human", {"sample": "100", "alternatives-from-sampling": "true", "maxtracks": "2"}, None),
    # UTR states + alternatives: transcripts that differ in a UTR end only often have EQUAL mean state probability (7 pairs among the
    # 18 of this record); which of two equals comes first follows the addresses of the reference's Gene objects -- falling in the
    # order of creation through the sampling loop of a record, restated as that in genes.cc: groupToGenes
    "human_utr_alt": ("human", {"UTR": "on", "sample": "30", "alternatives-from-sampling": "true"}, ("HS04636",)),
}


# --singlestrand=true (tests/golden/make_golden.py single): the 24-state model without shadow states, every piece decoded as it is and
# as its reverse complement, genes on opposite strands may overlap
SINGLE_CFGS = {
    "human": ("human", {"singlestrand": "true"}),                                              # default flags: soft-masking bonus
    "human_complete": ("human", {"singlestrand": "true", "genemodel": "complete", "softmasking": "0"}),
    "fly_sampled": ("fly", {"singlestrand": "true", "UTR": "off", "softmasking": "0"}),       # sample = 100: draws run forward, then reverse
    "fly_backward": ("fly", {"singlestrand": "true", "UTR": "off", "sample": "0", "strand": "backward"}),
    "fly_pieces": ("fly", {"singlestrand": "true", "UTR": "off", "sample": "0", "maxDNAPieceSize": "20000"}),  # cut finder + both runs per piece
    # alternatives from the sample in both runs: the genes of the reverse run are mirrored transcript by transcript
    "fly_alt": ("fly", {"singlestrand": "true", "UTR": "off", "softmasking": "0", "alternatives-from-sampling": "true", "maxtracks": "3"}),
}


# --noInFrameStop (tests/golden/make_golden_noinframestop.py): a gene whose CDS holds a stop codon put together by a long intron
NOINFRAMESTOP_CFGS = {
    "off": {"UTR": "off", "sample": "0", "softmasking": "0", "noInFrameStop": "false"},
    "on": {"UTR": "off", "sample": "0", "softmasking": "0", "noInFrameStop": "true"},
    "on_single": {"UTR": "off", "sample": "0", "softmasking": "0", "noInFrameStop": "true", "singlestrand": "true"},
    "on_sampled": {"UTR": "off", "softmasking": "0", "noInFrameStop": "true", "sample": "30"},
}


def inframe_stop_records():
    import gzip
    txt = gzip.open(os.path.join(GOLDEN, "inframe_stop.fa.gz"), "rt").read().split("\n")
    return [(txt[0][1:], txt[1]), (txt[2][1:], txt[3])]


def multiclass_path_case():
    """a 25 kb record (found by tests/soak_cli.py, seed 4025) whose OPTIMAL PATH under the human single-strand model depends on the
    reference's snippet cache across a GC-class step: (sequence, options, reference ln Viterbi, reference path)"""
    import gzip
    g = json.load(open(os.path.join(GOLDEN, "multiclass_path_case.json")))
    seq = gzip.open(os.path.join(GOLDEN, "multiclass_path_case.fa.gz"), "rt").read().split("\n")[1]
    return seq, g["options"], float(g["lnv"]), [tuple(p) for p in g["path"]]


def golden_single_gff(cfg):
    return open(os.path.join(GOLDEN, "golden_single_%s.gff" % cfg)).read().splitlines()


def sampled_records(cfg):
    names = SAMPLED_CFGS[cfg][2]
    recs = golden_inputs()
    if names is None:
        return recs
    byname = dict(recs)
    return [(k, byname[k]) for k in names]


def golden_sampled_gff(cfg):
    return open(os.path.join(GOLDEN, "golden_sampled_%s.gff" % cfg)).read().splitlines()


def gff_scores_apart(lines):
    """(lines with the score column masked, the scores) of GFF text: what is compared where the sample itself may differ"""
    struct, sc = [], []
    for l in lines:
        w = l.split("\t")
        if len(w) >= 9:
            sc.append(None if w[5] == "." else float(w[5]))
            w[5] = "*"
            struct.append("\t".join(w))
        else:
            struct.append(l)
    return struct, sc


def golden_sampled_paths(cfg):
    g = json.load(open(os.path.join(GOLDEN, "golden_sampled_paths_%s.json" % cfg)))
    return [[[tuple(st) for st in smp] for smp in r["samples"]] for r in g["records"]]


def golden_inputs():
    return read_fasta(os.path.join(GOLDEN, "inputs.fa"))


def golden_paths(cfg):
    g = json.load(open(os.path.join(GOLDEN, "golden_paths_%s.json" % cfg)))
    for r in g["records"]:
        r["lnv"] = float(r["lnv"])
        r["path"] = [tuple(p) for p in r["path"]]
    return g


def golden_gff(cfg):
    return open(os.path.join(GOLDEN, "golden_%s.gff" % cfg)).read().splitlines()


class _Piece(ctypes.Structure):
    _fields_ = [("seq", ctypes.c_char_p), ("len", ctypes.c_int64), ("init_kind", ctypes.c_int32), ("term_kind", ctypes.c_int32)]


_emu = None


def emu_decode(tables_ptr, seqs, S, cells=False, init_kind=0, term_kind=0, lib=None, forward=False, samples=0, seed=1, tss0=None, prep=False):
    """Run the device kernel bodies on the CPU (tests/emu/emu.cc).  Returns [(status, lnv, path, V, cls)]
    (forward=True: [(status, lnv, path, V, cls, F, lnP)] with the ln forward matrix F and ln P(sequence);
    samples=n: [(status, lnv, path, V, cls, F, lnP, [n sampled paths of (begin, end, type)])], drawn from one rand() stream over seqs)."""
    forward = forward or samples > 0
    global _emu
    if lib is not None:
        _emu_lib = ctypes.CDLL(lib)
    elif _emu is None:
        _emu = ctypes.CDLL(EMU_LIB)
    n = len(seqs)
    P = (_Piece * n)()
    keep = [s.encode() if isinstance(s, str) else s for s in seqs]
    for i, b in enumerate(keep):
        P[i].seq, P[i].len = b, len(b)
        P[i].init_kind = init_kind[i] if isinstance(init_kind, (list, tuple)) else init_kind
        P[i].term_kind = term_kind[i] if isinstance(term_kind, (list, tuple)) else term_kind
    lnv = np.zeros(n)
    st = np.zeros(n, dtype=np.int32)
    cap = max(1024, max(len(s) for s in seqs) // 4 + 16)
    po = np.zeros((n, cap, 3), dtype=np.int32)
    pn = np.zeros(n, dtype=np.int32)
    cls = np.zeros(n, dtype=np.int32)
    tot = sum(len(s) for s in seqs)
    C = np.zeros(tot * S) if cells else None
    FW = np.zeros(tot * S) if forward else None
    lnF = np.zeros(n)
    E = _emu_lib if lib is not None else _emu
    E.emu_prep_keep(1 if prep else 0)  # (emu_prep below reads what this decode's preparation stage left)
    E.emu_set_sampling(samples, seed)
    if tss0 is not None:  # [(forward, reverse) or None per piece]: the value of the TSS window at base 0 an earlier sequence left (BatchView::tss0)
        tv = np.array([[float('nan')] * 2 if t is None else list(t) for t in tss0], dtype=np.float64)
        E.emu_set_tss0(tv.ctypes.data_as(ctypes.c_void_p), len(tss0))
    else:
        E.emu_set_tss0(None, 0)
    rc = E.emu_decode(tables_ptr, P, n, lnv.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p),
                         po.ctypes.data_as(ctypes.c_void_p), cap, pn.ctypes.data_as(ctypes.c_void_p),
                         C.ctypes.data_as(ctypes.c_void_p) if cells else None, cls.ctypes.data_as(ctypes.c_void_p),
                         FW.ctypes.data_as(ctypes.c_void_p) if forward else None, lnF.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    out, w = [], 0
    for i, s in enumerate(seqs):
        V = C[w:w + len(s) * S].reshape(len(s), S) if cells else None
        Fm = FW[w:w + len(s) * S].reshape(len(s), S) if forward else None
        w += len(s) * S
        rec = (int(st[i]), float(lnv[i]), [tuple(int(x) for x in po[i, k]) for k in range(pn[i])], V, int(cls[i]))
        if samples:
            buf = np.zeros((max(1024, len(s) // 2 + 16), 3), dtype=np.int32)
            sm = []
            for it in range(samples):
                k = E.emu_sample_get(i, it, buf.ctypes.data_as(ctypes.c_void_p), len(buf))
                assert 0 <= k <= len(buf)
                sm.append([tuple(int(x) for x in buf[q]) for q in range(k)])
            out.append(rec + (Fm, float(lnF[i]), sm))
        else:
            out.append(rec + (Fm, float(lnF[i])) if forward else rec)
    E.emu_set_sampling(0, 1)
    return out


def emu_state_type(tables_ptr, s):
    return _emu.emu_state_type(tables_ptr, s)


# branches of the candidate kernel's evaluation pass (kernels.h: candTile, EmuCand), in the order of the emulator's counters
CAND_COVERAGE = ("tiles", "tiles_gt_wave", "tiles_gt_dcap", "rounds_a_gt_wave", "rounds_e_gt_wave", "rounds_a0", "rounds_e0",
                 "chunks_a_cont", "chunks_e_cont", "full_flush", "full_flush_move", "tail_flush", "max_ns")


def _emu_of(lib):
    global _emu
    if lib is not None:
        return ctypes.CDLL(lib)
    if _emu is None:
        _emu = ctypes.CDLL(EMU_LIB)
    return _emu


def _repeat(motif, n):
    return (motif * (n // len(motif) + 1))[:n]


def _gc_dna(n, gc, seed):
    rng = random.Random(seed)
    return "".join(rng.choice("GC") if rng.random() < gc else rng.choice("AT") for _ in range(n))


def cand_edge_cases():
    """[(name, sequence)] made for the evaluation pass of the candidate kernel (kernels.h: candTile, pass 2); tests/test_emu_cand.py
    checks that they reach every branch of it.
    - motif repeats that put reverse-strand exon ends next to dense splice sites: tiles of more than DCAP (base, state) pairs,
      rounds with several chunks of either class, pairs whose candidates run on from one chunk into the next;
    - pieces of 64-600 bases of short repeats: every exon pair of such a piece also has a candidate that starts at base 0 and needs
      the general formula, so that a round queues more than a wavefront of them (the slow queue is flushed full, the rest moved);
    - a record whose GC content steps from a low class to a high one: some piece of the batch has two classes (MULTI)"""
    rnd = lambda n, seed: random_dna(n, 9000 + seed)
    recs = [
        ("accTac_rep", rnd(300, 1) + _repeat("ACCTAC", 4800) + rnd(300, 2)),
        ("ttacta_rep", rnd(200, 3) + _repeat("TTACTACTA", 3600) + rnd(400, 4)),
        ("gtagctac_rep", rnd(500, 5) + _repeat("GTAGCTAC", 3200) + rnd(100, 6)),
    ]
    # short pieces: queue fills of 64 and more (a bounded search over motifs and lengths, driven by the emulator's counters)
    for motif, n in (("CATA", 600), ("CATA", 160), ("ATAC", 160), ("ATGGT", 600), ("ATGAGT", 100), ("CAGT", 160), ("ACTGAC", 128),
                     ("ACCTAC", 200), ("TTACTACTA", 64), ("GTAGCTAC", 96)):
        recs.append(("%s_%d" % (motif.lower(), n), _repeat(motif, n)))
    recs += [("rand_%d" % n, rnd(n, n)) for n in (64, 65, 127, 160)]
    recs.append(("twoclass", _gc_dna(9000, 0.30, 9101) + _gc_dna(7000, 0.66, 9102)))
    return recs


def cand_edge_long(n=260000):
    """one record of n bases of random DNA with blocks of the motif repeats of cand_edge_cases().  At AUGX_SEG_LEN=100000 it is cut into
    three segments (at 86 656 and 173 312 for the default n), and two of the blocks lie across the cuts: the trellis fix-ups there size
    their check window from the candidate kernel's tile minima (BatchView::tileMinEop)"""
    s = random_dna(n, 9200)
    for at, motif in ((83000, "ACCTAC"), (130000, "CATA"), (170000, "TTACTACTA")):
        s = s[:at] + _repeat(motif, 6000) + s[at + 6000:]
    return s


def emu_cand_coverage(lib=None, reset=False):
    """{counter: value} of the branches candTile's pass 2 took in the emulator `lib` since its last reset (max_ns: the largest
    fill of the slow queue); reset=True clears them afterwards"""
    E = _emu_of(lib)
    out = (ctypes.c_longlong * 64)()
    n = E.emu_cand_coverage(out)
    assert n == len(CAND_COVERAGE), n
    if reset:
        E.emu_cand_coverage_reset()
    return dict(zip(CAND_COVERAGE, out[:n]))


def emu_cand_coverage_reset(lib=None):
    _emu_of(lib).emu_cand_coverage_reset()


def emu_slowq_at(lib=None):
    """the slow-queue threshold the emulator `lib` was built with (kernels.h: SLOWQ_AT)"""
    return _emu_of(lib).emu_slowq_at()


def emu_block_size(tables_ptr, lib=None):
    """block size of the candidate / trellis kernels for this model (layout.h: chooseBlockSize, AUGX_BLK applies)"""
    return _emu_of(lib).emu_block_size(tables_ptr)


def format_gff_sampled(model, recs, paths, samples):
    """GFF text of the product's gene-structure stage with posterior probabilities (augx_format_gff_sampled): paths[k] the Viterbi
    path [(begin, end, state, type)], samples[k] the sampled paths [(begin, end, type)] of record k"""
    import augustus_amd as ax
    L = ax.lib()
    out, gid = [], 1
    for k, ((name, seq), path, smp) in enumerate(zip(recs, paths, samples)):
        sts = (_St * max(1, len(path)))()
        for i, (b, e, st, t) in enumerate(path):
            sts[i].begin, sts[i].end, sts[i].state, sts[i].type = b, e, st, t
        arrs, ns, ptrs = [], (ctypes.c_int * max(1, len(smp)))(), (ctypes.POINTER(_St) * max(1, len(smp)))()
        for q, sp in enumerate(smp):
            a = (_St * max(1, len(sp)))()
            for i, (b, e, t) in enumerate(sp):
                a[i].begin, a[i].end, a[i].state, a[i].type = b, e, 0, t
            arrs.append(a)
            ns[q] = len(sp)
            ptrs[q] = ctypes.cast(a, ctypes.POINTER(_St))
        buf = ctypes.create_string_buffer(16 << 20)
        ng = ctypes.c_int()
        rc = L.augx_format_gff_sampled(model._h, name.encode(), seq.encode(), ctypes.c_int64(len(seq)), sts, len(path), len(smp), ptrs, ns,
                                       gid, buf, ctypes.c_int64(16 << 20), ctypes.byref(ng))
        assert rc == 0, ax.last_error() if hasattr(ax, "last_error") else rc
        out.append("# ----- prediction on sequence number %d (length = %d, name = %s) -----" % (k + 1, len(seq), name))
        out.append("#")
        st = model.option("strand")
        out.append("# Predicted genes for sequence number %d on %s" % (k + 1, "forward strand" if st == "forward" else "reverse strand" if st == "backward" else "both strands"))
        out += buf.value.decode().splitlines()
        if ng.value == 0:
            out.append("# (none)")
        gid += ng.value
        out.append("#")
    return out[:-1]


def format_gff(model, recs, paths):
    """GFF text of the product's gene-structure stage for externally supplied paths (augx_format_gff)."""
    import augustus_amd as ax
    L = ax.lib()
    L.augx_format_gff.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p,
                                  ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int)]
    out, gid = [], 1
    for k, ((name, seq), path) in enumerate(zip(recs, paths)):
        sts = (_St * max(1, len(path)))()
        for i, (b, e, s, t) in enumerate(path):
            sts[i].begin, sts[i].end, sts[i].state, sts[i].type = b, e, s, t
        buf = ctypes.create_string_buffer(16 << 20)
        ng = ctypes.c_int()
        rc = L.augx_format_gff(model._h, name.encode(), seq.encode(), len(seq), sts, len(path), gid, buf, 16 << 20, ctypes.byref(ng))
        assert rc == 0, L.augx_last_error()
        out.append("# ----- prediction on sequence number %d (length = %d, name = %s) -----" % (k + 1, len(seq), name))
        out.append("#")
        st = model.option("strand")
        out.append("# Predicted genes for sequence number %d on %s" % (k + 1, "forward strand" if st == "forward" else "reverse strand" if st == "backward" else "both strands"))
        out += buf.value.decode().splitlines()
        if ng.value == 0:
            out.append("# (none)")
        gid += ng.value
        out.append("#")
    return out[:-1]


def gff_body(stdout_text):
    """Prediction part of an augustus stdout, as the reference's own test filter does (tests/short/utils/aug_out_filter.py)."""
    lines = stdout_text.splitlines()
    i0 = [k for k, l in enumerate(lines) if l.startswith("# ----- prediction")][0]
    return [l for l in lines[i0:] if not l.startswith("# command line")][:-1]


# ---------------------------------------------------------------------------------------------------
# the preparation stage of a decode, array by array (tests/test_emu_prep.py, tests/test_gpu_prep.py)
# ---------------------------------------------------------------------------------------------------
def emu_prep(piece, which, plane=0, lib=None):
    """array `which` (a name of augustus_amd.PREP_ARRAYS) of one piece as the preparation stage of the last emu_decode(..., prep=True)
    left it: the emulator's counterpart of Batch.prep, same layout, same refusals"""
    import augustus_amd as ax
    E = _emu_of(lib)
    E.emu_prep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    return ax.prep_fetch(lambda w, pl, out, cap, nb: E.emu_prep(piece, w, pl, out, cap, nb), which, plane)


def emu_prep_runs(piece, lib=None):
    """runs of equal GC-window class of one piece of the last emu_decode(..., prep=True), as the device's stairs kernel counts them"""
    return _emu_of(lib).emu_prep_runs(piece)


def emu_prep_off(piece, lib=None):
    """first slot of piece `piece` in the batch of the last emu_decode(..., prep=True) (piece = number of pieces: the batch's slots)"""
    E = _emu_of(lib)
    E.emu_prep_off.restype = ctypes.c_longlong
    return E.emu_prep_off(piece)


def stair_runs(lib=None):
    """layout.h: STAIR_RUNS, the runs of window classes the device's stairs kernel holds (a piece with more goes to the host)"""
    return _emu_of(lib).emu_stair_runs()


def scan_block(lib=None):
    """layout.h: SCAN_T, slots per block of the device's prefix scans"""
    return _emu_of(lib).emu_scan_block()


def emu_gc_win(tables_ptr, lib=None):
    return _emu_of(lib).emu_gc_win(tables_ptr)


def emu_n_classes(tables_ptr, lib=None):
    return _emu_of(lib).emu_n_classes(tables_ptr)


def _ag_window(win, k):
    """a window of A with k G spread evenly, a G first"""
    return ["G" if (i * k) // win != ((i - 1) * k) // win else "A" for i in range(win)]


def _toggle_seq(win, k, n, want):
    """n bases whose GC windows hold k or k - 1 G: the first window is _ag_window(win, k); every further base copies the base one window
    back, so that the window that begins at s holds what the one before it held -- except at the window starts in `want` (ascending,
    each put off until the base that leaves is of the kind that can be turned), where the base that enters is the other kind than the
    base that leaves: a G leaves and an A enters (k -> k - 1), next time an A leaves and a G enters (k - 1 -> k), and so on.
    Returns (sequence, the window starts where the count really changed)."""
    seq = _ag_window(win, k)
    full, done, j = True, [], 0
    for i in range(win, n):
        s, b = i - win + 1, seq[i - win]
        if j < len(want) and s >= want[j] and b == ("G" if full else "A"):
            b = "A" if full else "G"
            full = not full
            done.append(s)
            j += 1
        seq.append(b)
    return "".join(seq), done


def _class_boundary(m):
    """(k, class of a window of A with k G, class with k - 1 G) at a boundary between two GC classes of model m, by bisection on the
    emulator's window classes (it depends on the model files)"""
    win = emu_gc_win(m.tables_ptr)

    def cls(k):
        emu_decode(m.tables_ptr, ["".join(_ag_window(win, k))], m.n_states, prep=True)
        return int(emu_prep(0, "gcRaw")[0])
    lo, hi = 0, win // 2
    c0 = cls(lo)
    assert cls(hi) != c0, "a window of A and one that is half G have one GC class"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if cls(mid) == c0:
            lo = mid
        else:
            hi = mid
    return hi, cls(hi), c0


_prep_cases = {}

# the records of prep_edge_cases that every configuration decodes (the others: the models with two or more GC classes whose window
# is GCwinsize, i.e. the human ones)
PREP_COMMON = ("planes_unordered", "n_window", "blocks_64", "sites_after_blocks_64", "blocks_68", "blocks_128", "blocks_132")
TINY_LENS = (1, 7, 255, 1014, 1015, 1016, 2039)


def prep_edge_cases(m, key):
    """[(name, sequence)] made for the preparation stage of a decode (decoder.hip: the kernels before kCand), in batch order;
    tests/test_emu_prep.py asserts from the emulator's arrays that each record meets the condition it is named for.  `key` names the
    configuration of model m (the records are built once per configuration).
    - runs_over / runs_at / runs_at_plus1: more runs of GC-window classes than the device's stairs kernel holds (layout.h: STAIR_RUNS;
      the host settles the piece), exactly as many, one more.  The window count of G moves across a class boundary and back every few
      bases (_toggle_seq); the two others are the same sequence cut where the run count reaches the limit;
    - one_plane_after_smoothing, short_run_first, step_999 / step_1000: a run of the other class of 999 positions or fewer between two
      runs of one class is dissolved, one of 1000 stays; a short run right after run 0 (one window);
    - planes_unordered: stretches longer than the GC window whose GC content falls from 0.72 to 0.24: the classes appear high to low,
      so the planes (numbered by first appearance) are not in class order;
    - below_window .. window_plus_300: pieces shorter than, as long as, and a little longer than the GC window; class_in_block_1_only:
      the second class shows in the windows of one block of 256 slots only;
    - blocks_*: pieces of exactly 64, 68, 128 and 132 scan blocks (a piece takes len + 9 slots rounded up to a chunk of 4 blocks);
    - tiny_*: a site-dense motif repeat cut to lengths around a chunk; sites_*: site-dense neighbours of the pieces whose pad is short
      (1015 and 16 375 bases leave 9 pad slots) and a repeat with a period coprime to the scan block;
    - n_window (windows without a nucleotide), softmasked (lower-case stretches: the soft-mask count)."""
    if key in _prep_cases:
        return _prep_cases[key]
    win, ncls = emu_gc_win(m.tables_ptr), emu_n_classes(m.tables_ptr)
    rnd = lambda n, seed: random_dna(n, 9300 + seed)
    unit = "ACCTAC" + "TTACTACTA" + "GTAGCTAC" + "CATA" + "ATGGT" + "ATGAGT" + "CAGT" + "ACTGAC" + "T"  # the motifs of cand_edge_cases
    assert len(unit) % 2 == 1  # (coprime to the scan block of 256 slots: every site kind lands on every slot of a block)
    gcs = (0.72, 0.66, 0.62, 0.58, 0.54, 0.50, 0.46, 0.42, 0.38, 0.34, 0.30, 0.24)
    stretch = max(12000, win + 2000)
    common = {
        "planes_unordered": "".join(_gc_dna(stretch, gc, 9400 + i) for i, gc in enumerate(gcs)),
        "n_window": n_window_record()[1],
        "blocks_64": rnd(16375, 1), "blocks_68": rnd(16376, 2), "blocks_128": rnd(32759, 3), "blocks_132": rnd(32760, 4),
        "sites_after_blocks_64": _repeat("ACCTAC", 700),
    }
    recs = []
    if key.startswith("human"):
        k, c_full, c_less = _class_boundary(m)
        # (an odd number of changes: the last 3500 windows keep the other class, the piece has two planes after the smoothing)
        over, tg = _toggle_seq(win, k, win + 30000, list(range(1, 26000, 4)) + [26500])
        assert len(tg) % 2 == 1
        limit = stair_runs()
        assert len(tg) > limit + 8
        # run r begins at window start tg[r - 1]: a piece cut to win + s bases has the window starts 0 .. s
        recs += [("runs_over", over), ("runs_at", over[:win + tg[limit - 2]]), ("runs_at_plus1", over[:win + tg[limit - 1]])]
        recs.append(("one_plane_after_smoothing", _toggle_seq(win, k, win + 4000, [500, 560, 1200, 1500, 2400, 2410])[0]))
        for L in (999, 1000):  # a window start where a G leaves, and L starts later an A
            s1 = next(s for s in range(1500, 1500 + win) if _toggle_seq(win, k, win + s + L + 1, [s, s + L])[1] == [s, s + L])
            recs.append(("step_%d" % L, _toggle_seq(win, k, win + s1 + L + 2500, [s1, s1 + L])[0]))
        recs.append(("short_run_first", _toggle_seq(win, k, win + 2500, [1, 300])[0]))
        recs += [("below_window", rnd(win - 1, 5)), ("at_window", rnd(win, 6)),
                 ("window_plus_1", _toggle_seq(win, k, win + 1, [1])[0]), ("window_plus_300", _toggle_seq(win, k, win + 300, [100, 200])[0])]
        # the only windows of the second class lie in the piece's second block of 256 slots (kClassFinal folds the blocks of a piece,
        # one per lane); they are the last run, which the smoothing keeps however short
        recs.append(("class_in_block_1_only", _toggle_seq(win, k, win + 300, [260])[0]))
        recs.append(("sites_first", _repeat("TTACTACTA", 900)))
        for n in TINY_LENS:
            recs.append(("tiny_%d" % n, _repeat("GTAGCTAC" + "ATGGT" + "CATA", n)))
            if n == 1015:
                recs.append(("sites_after_tiny_1015", _repeat("CATA", 600)))
        sm = list(rnd(9000, 7))
        for a, b in ((0, 40), (700, 1900), (1023, 1025), (4000, 4001), (8200, 9000)):
            sm[a:b] = "".join(sm[a:b]).lower()
        recs += [("sites_all_alignments", _repeat(unit, 256 * len(unit) + 100)), ("softmasked", "".join(sm))]
    recs += [(name, common[name]) for name in PREP_COMMON]
    _prep_cases[key] = recs
    return recs


def prep_one_plane_piece(m, n):
    """n bases (more than the GC window + 3000) whose windows change class six times in short runs that the smoothing dissolves: the
    record one_plane_after_smoothing of prep_edge_cases at another length"""
    win = emu_gc_win(m.tables_ptr)
    assert n >= win + 3000
    return _toggle_seq(win, _class_boundary(m)[0], n, [500, 560, 1200, 1500, 2400, 2410])[0]


PREP_CFGS = {**{k: GOLDEN_CFGS[k] for k in ("human", "human_utr")}, "nasonia": MORE_CFGS["nasonia"],
             "maize": ("maize", {"UTR": "off", "sample": "0", "softmasking": "0"})}


def prep_arrays(fetch, piece, dense):
    """every array of the preparation stage of one piece through fetch(piece, which, plane): [(which, plane, array)], the arrays with
    one plane per GC class of the piece once per plane, planeCls cut to the planes the piece has"""
    npl = int(fetch(piece, "nPlanes", 0))
    out = [("nPlanes", 0, np.asarray(npl))]
    for which in ("cls", "planeCls", "listCnt", "code", "cnt", "nsm", "gcRaw", "gcPlane", "sig", "gate") + (("ufx", "ucnt") if dense else ()):
        a = fetch(piece, which, 0)
        out.append((which, 0, a[:npl] if which == "planeCls" else a))
    for which in ("fx", "plsR"):
        out += [(which, pl, fetch(piece, which, pl)) for pl in range(npl)]
    return out


def prep_first_diff(got, want):
    """None if the two arrays are equal bit for bit (doubles through their bit patterns: -inf, signed zeros and NaN payloads count),
    else a text that names the first position (row = slot or base) and the field that differ"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return "dtype / shape %s %s against %s %s" % (got.dtype, got.shape, want.dtype, want.shape)
    a, b = (x.view(np.uint64) if x.dtype == np.float64 else x for x in (np.ascontiguousarray(got), np.ascontiguousarray(want)))
    if np.array_equal(a, b):
        return None
    bad = np.argwhere(np.atleast_1d(a != b))
    first = tuple(int(x) for x in bad[0])
    return "%d of %d values differ, first at position %d field %d: %r against %r" % (
        len(bad), a.size, first[0], first[1] if len(first) > 1 else 0, np.atleast_1d(got)[first], np.atleast_1d(want)[first])


# ---------------------------------------------------------------------------------------------------
# the far-window and overflow paths of the trellis and forward kernels (tests/test_emu_trellis.py, tests/test_gpu_trellis.py)
# ---------------------------------------------------------------------------------------------------
# kernels.h: EmuTrellis, in the order of the emulator's counters ("*_0".."*_3": per list, sel 0 laVal, 1 lrVal, 2 ldVal, 3 rdVal)
TRELLIS_COVERAGE = (("chunk_hbm", "chunk_straddle") + tuple("slow_list_%d" % i for i in range(4)) + ("slow_vig",)
                    + tuple("pay_top_%d" % i for i in range(4)) + tuple("pay_top1_%d" % i for i in range(4))
                    + ("pay_viglo", "pay_viglo1", "slow_dead", "slow_dead_cut", "slow_mode1", "slow_mode2", "slow_mode3", "slow_past_jump",
                       "slow_multi", "list_past_jump", "flush_cmp", "flush_cmp_bad", "longv_read", "tile_full", "jump_restage",
                       "fix_converged", "fix_gaveup", "p3_converged", "p3_at_seam", "p3_to_end", "m3_tiles", "fin_overrun", "fin_covered",
                       "fin_to_end", "fin_seam", "fwd_gt_ntw", "fwd_nonrt_gt_ntw", "fwd_at_hbm", "fwd_max_cell", "fwd_max_sum",
                       "fwd_trn_multi", "fwd_trn_single", "fwd_col0", "fwd_heated_over"))
SMALLWIN_EMU_LIB = os.path.join(ROOT, "build", "libaugx_emu_smallwin.so")
SMALLWIN_LIB = os.path.join(ROOT, "augustus_amd", "libaugx_smallwin.so")


def emu_trellis_coverage(lib=None, reset=False):
    """{counter: value} of the data paths the trellis, its segment bookkeeping and the forward kernel took in the emulator `lib` since
    its last reset (fwd_max_cell, fwd_max_sum: maxima); reset=True clears them afterwards"""
    E = _emu_of(lib)
    out = (ctypes.c_longlong * 128)()
    n = E.emu_trellis_coverage(out)
    assert n == len(TRELLIS_COVERAGE), n
    if reset:
        E.emu_trellis_coverage_reset()
    return dict(zip(TRELLIS_COVERAGE, out[:n]))


def emu_trellis_coverage_reset(lib=None):
    _emu_of(lib).emu_trellis_coverage_reset()


def emu_trellis_windows(lib=None):
    """the trellis windows the emulator `lib` was built with: {ITEM_CAP, LIST_WIN, VIG_WIN, LIST_AHEAD, NTW} (kernels.h), and
    FWD_SUM_TERMS, the terms of 1.0 a fixed-point sum of the forward kernels holds (dp.h); BT_ROUND / BT_ROUND_DENSE: the bases of a
    chain run that one round of loads of the back-trace covers (kernels.h: backtracePiece / dense.h: denseBacktracePiece)"""
    out = (ctypes.c_int * 8)()
    _emu_of(lib).emu_trellis_windows(out)
    return dict(zip(("ITEM_CAP", "LIST_WIN", "VIG_WIN", "LIST_AHEAD", "NTW", "FWD_SUM_TERMS", "BT_ROUND", "BT_ROUND_DENSE"), out[:8]))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def emu_model_dims(tables_ptr, lib=None):
    """{d, max_exon_len, W, dStateLen, n_classes, fwd_cell_candidates} of a loaded model (include/augx.h: augx_tables; dStateLen as
    the kernels get it; fwd_cell_candidates: the most candidates one forward cell can have, layout.h: forwardCellCandidates)"""
    out = (ctypes.c_longlong * 8)()
    _emu_of(lib).emu_model_dims(tables_ptr, out)
    return dict(zip(("d", "max_exon_len", "W", "dStateLen", "n_classes", "fwd_cell_candidates"), out[:6]))


def trellis_edge_cases():
    """[(name, sequence)] made for the data paths of the trellis and forward kernels that ordinary DNA almost never takes (kernels.h:
    trellisItems, loadTileThread, forwardPiece); tests/test_emu_trellis.py asserts from the emulator's counters (EmuTrellis) that they
    take them.  Found by a search over motifs driven by those counters; every record is 25 kb or shorter.
    - ag_rich, ac_rich: random purines / random {A, C}: reading frames without a stop codon whose exon candidates read acceptor
      (laVal, list 0) and reverse donor (lrVal, list 1) values more than LIST_WIN - LIST_AHEAD entries back, from HBM;
    - gt_cag, ct_tac: 600 donor sites two bases apart, then acceptors (and the same on the reverse strand): the short-intron candidates
      read ldVal (list 2) and rdVal (list 3) back; needs an intron d of more than twice LIST_WIN - LIST_AHEAD bases;
    - atg_ggt: 300 start codons in one open frame, then 400 donor sites: initial-exon candidates whose igenic predecessor lies
      0 .. 2100 bases back, among them pay == vigLo and pay == vigLo + 1 of every block alignment;
    - cag_many: about 4000 in-frame acceptors for the cells of one donor site: thousands of candidates summed into one forward cell, tiles
      of 30 000 candidates (beyond ITEM_CAP, beyond the threads of the forward kernel);
    - cag_N_cag: the same reading frame across a run of 3600 N, which the trellis jumps over: predecessors (list and igenic) older
      than the jump;
    - orf12k: one single-exon gene of 12 kb (igenic predecessor 12 kb back);
    - multi_far: the far blocks between a stretch of low and one of high GC content: a piece with two GC classes under the human model"""
    rng8 = np.random.default_rng(8)
    ag = "".join(rng8.choice(list("AG"), size=20000))
    pre = post = "ACGT" * 500
    return [
        ("ag_rich", ag),
        ("ac_rich", random_dna(20000, 77, "AC")),
        ("gt_cag", pre + "GT" * 600 + "CAG" * 40 + post),
        ("ct_tac", pre + "CT" * 600 + "TAC" * 40 + post),
        ("atg_ggt", pre + "ATG" * 300 + "GGT" * 400 + post),
        ("cag_many", "ACGT" * 250 + "ATG" + "CAG" * 3990 + "GTAAGT" + post),
        ("cag_N_cag", pre + "ATG" + "CAG" * 1500 + "N" * 3600 + "CAG" * 1500 + "GTAAGT" + post),
        ("orf12k", random_dna(1000, 3) + "ATG" + "GCC" * 4000 + "TAA" + random_dna(1000, 4)),
        ("multi_far", _gc_dna(9000, 0.30, 9101) + "CT" * 600 + "TAC" * 40 + "ACGT" * 200 + "GT" * 600 + "CAG" * 40 + ag[:3000] + _gc_dna(9000, 0.66, 9102)),
    ]


def trellis_edge_long(n=390000):
    """one record of n bases that AUGX_SEG_LEN=77000 cuts into five segments under the human model (a segment is at least five check
    windows of maxexonlength long): random DNA with far-predecessor blocks of trellis_edge_cases() across the first and the second cut
    -- reading frames and their candidates span the seams --, a run of N from before the third cut to beyond the limit of the fix-up
    that starts there, which therefore gives up (a dead start cannot converge inside a run of N) and is continued by pass 3, and a run
    of 7000 N across the fourth cut: the fix-up that starts in it and the continuation settle on the truth in the same tiles behind
    it, and the continuation, which must not stop on the other run's seam, runs over it (found by a search over the length of that run)"""
    s = random_dna(n, 9500)
    cuts = [((n + 63) // 64 * k // 5) * 64 for k in range(1, 5)]
    blocks = dict(trellis_edge_cases())
    for at, block in ((cuts[0] - 7000, blocks["cag_many"][1000:-2000]), (cuts[1] - 3000, blocks["ag_rich"][:6000]),
                      (cuts[2] - 9000, "N" * (9000 + n // 5 - 14000)), (cuts[3] - 2000, "N" * 7000)):
        s = s[:at] + block + s[at + len(block):]
    assert len(s) == n
    return s


# ---------------------------------------------------------------------------------------------------
# the rare data paths of the dense kernels (tests/test_emu_dense.py, tests/test_gpu_dense.py)
# ---------------------------------------------------------------------------------------------------
# dense.h: EmuDense, in the order of the emulator's counters ("at63_k" / "at64_k": per caller of denseAt, 0 a record of kCand, 1 a UTR
# exon candidate, 2 a fixed-lag state)
DENSE_COVERAGE = (("desc_multi_unit", "desc_gt_waves", "max_total", "last_half_empty", "total_exact", "max_block_descs", "desc_hbm",
                   "pre_1", "pre_2", "pre_3", "extra_tf", "extra_tm", "extra_fs", "extra_rt", "extra_la", "mid_1", "mid_0", "mid_neg",
                   "tail3_right", "tail3_left") + tuple("at63_%d" % i for i in range(3)) + tuple("at64_%d" % i for i in range(3))
                  + ("nonrt_gt_ntw", "max_rt", "redo_cells", "redo_live", "chain_general", "lateacc_false", "all_n", "trn_hbm", "trn_lds",
                     "max_anc_utr", "bt_step2", "bt_run_base1", "bt_utr_chunks", "bt_rec_chunks", "bt_tie_eop", "bt_tie_anc", "bt_near_pass"))
DENSE_MAXIMA = ("max_total", "max_block_descs", "max_rt", "max_anc_utr")  # (maxima, not counts)


def emu_dense_coverage(lib=None, reset=False):
    """{counter: value} of the data paths the dense kernels (dense.h: densePiece, denseBacktracePiece) took in the emulator `lib` since
    its last reset (DENSE_MAXIMA: maxima); reset=True clears them afterwards"""
    E = _emu_of(lib)
    out = (ctypes.c_longlong * 128)()
    n = E.emu_dense_coverage(out)
    assert n == len(DENSE_COVERAGE), n
    if reset:
        E.emu_dense_coverage_reset()
    return dict(zip(DENSE_COVERAGE, out[:n]))


def emu_dense_coverage_reset(lib=None):
    _emu_of(lib).emu_dense_coverage_reset()


def emu_dense_dims(blk, lib=None):
    """what the dense kernels of the emulator `lib` derive from the build at block size blk: {UDCAP: descriptors of a block staged in
    LDS, UNIT: candidates of a unit (UH * WAVE), CAND_WAVES: candidate wavefronts, NTW: threads of the record passes, BT_STEP: bases
    per step of a chain run of the back-trace}"""
    out = (ctypes.c_int * 8)()
    _emu_of(lib).emu_dense_dims(blk, out)
    return dict(zip(("UDCAP", "UNIT", "CAND_WAVES", "NTW", "BT_STEP"), out[:5]))


def emu_dense_lags(tables_ptr, lib=None):
    """how far the fixed-lag states of a loaded model look back in densePiece: (longdss, longass, equalD)"""
    out = (ctypes.c_int * 4)()
    _emu_of(lib).emu_dense_lags(tables_ptr, out)
    return tuple(out[:3])


DENSE_PREFIX_LENS = (1, 2, 3, 4, 5, 7, 31, 32, 33, 63, 64, 65, 127, 129, 1022, 1023, 1024, 1025)
# (index of a state of the twin's path of HS04636 under the human model with UTR states, bases behind its end at which the record is cut)
_DENSE_CUTS = ((3, 0), (5, 1), (11, 1), (14, 3), (19, 5), (28, 4), (34, 0), (41, 1))
_dense_cases = None


def dense_edge_cases():
    """[(name, sequence)] made for the data paths of the dense kernels that ordinary DNA rarely takes (dense.h: densePiece, utrPass,
    denseBacktracePiece); tests/test_emu_dense.py asserts from the emulator's counters (EmuDense) that they take them.  Found by a
    search over motifs driven by those counters; every record is 25 kb or shorter.
    - cag_dense: 2500 acceptor sites three bases apart: UTR exon cells with up to 1157 candidates under the human model -- descriptors of
      more units of 128 candidates than there are candidate wavefronts, so that a wavefront takes two units of one descriptor;
    - taa_after_gene, aataaa_after_gene: a gene, then stop codons / poly-A signals at every third (sixth) base: 3' UTR exons with up to
      1833 candidates, right- and left-truncated 3' UTRs (the tail distribution), the descriptors' pre-evaluated candidates (nPre 1..3);
    - tttatt: reverse poly-A signals: candidates that are truncated reverse signals, two ancestors of one predecessor end with equal value;
    - cat_dense, ac_tta: reverse acceptors / an AC stretch then reverse stops: middle parts of length 1, 0 and below 0, blocks with more
      records than the record passes have threads; ac_tta has two GC classes under the human model;
    - cag_many (helpers.trellis_edge_cases) and its reverse complement: 3990 in-frame acceptors before one donor site;
    - cut_*: the golden record HS04636 cut a few bases behind the end of a state of the oracle twin's path: the right-truncated 3' UTR
      cell of the last base is made again from predecessors of its own block (redoBlock), which are alive there;
    - prefix_n: the first n bases of HS04636 for the n of DENSE_PREFIX_LENS: the edges of a block (2, 4, 8), of the 32 bases of a group
      of the descriptor kernel, of the ring of 64 columns and of a chunk of 1024 slots;
    - N_1, N_2, N_5, N_300: pieces of N only (short-circuited by densePiece); gene_N_runs: HS04636 with runs of 1, 2, 5 and 300 N in it;
    - twoclass_gene: HS04636 between a stretch of low and one of high GC content: two GC classes under the human model, the transition
      terms of every cell come from HBM"""
    global _dense_cases
    if _dense_cases is not None:
        return list(_dense_cases)
    import augustus_amd as ax
    by = dict(golden_inputs())
    gene = by["HS04636"]
    tr = dict(trellis_edge_cases())
    acgt = "ACGT" * 500
    recs = [
        ("cag_dense", acgt + "CAG" * 2500 + acgt),
        ("taa_after_gene", gene + "TAA" * 2500),
        ("tttatt", "TTTATT" * 1200),
        ("aataaa_after_gene", gene + "AATAAA" * 1200),
        ("cat_dense", acgt + "CAT" * 2500 + acgt),
        ("ac_tta", random_dna(6000, 5, "AC") + "TTA" * 1500),
        ("cag_many", tr["cag_many"]),
        ("cag_many_rc", revcomp(tr["cag_many"])),
    ]
    m = ax.Model(config_path(), "human", UTR="on")
    rc, _, path, _, _ = twin_decode(m.tables_ptr, gene, m.n_states)
    assert rc == 0 and len(path) > max(i for i, _ in _DENSE_CUTS), len(path)
    assert len(_DENSE_CUTS) <= 16
    for i, k in _DENSE_CUTS:
        n = path[i][1] + 1 + k  # (path: 1-based begin and end of the state = index of its last base)
        assert 2 <= n <= len(gene)
        recs.append(("cut_%d_%d" % (i, k), gene[:n]))
    recs += [("prefix_%d" % n, gene[:n]) for n in DENSE_PREFIX_LENS]
    recs += [("N_%d" % n, "N" * n) for n in (1, 2, 5, 300)]
    recs.append(("gene_N_runs", gene[:3000] + "N" + gene[3001:5000] + "NN" + gene[5002:6000] + "N" * 5 + gene[6005:7000] + "N" * 300 + gene[7300:]))
    recs.append(("twoclass_gene", _gc_dna(7000, 0.30, 9101) + gene + _gc_dna(7000, 0.66, 9102)))
    assert max(len(s) for _, s in recs) <= 25000 and len(recs) <= 42
    _dense_cases = recs
    return list(recs)


BACKTRACE_EDGE_LENS = sorted(set(range(1, 301)) | {256 * k + d for k in range(1, 32) for d in (-1, 0, 1, 2)})


def dense_backtrace_prefixes(kmax=31):
    """[(name, sequence)]: the first n bases of the golden record softmask_all for n = 1..300 and n = 256 k + d, k = 1..kmax, d in
    {-1, 0, 1, 2}: one intergenic run of n - 1 bases under the models of tests/test_emu_dense.py (the caller asserts that from the twin's
    path): the chain runs of denseBacktracePiece that end on, one before and one after the last base of a step of 256, and at base 1"""
    src = dict(golden_inputs())["softmask_all"]
    lens = [n for n in BACKTRACE_EDGE_LENS if n <= 256 * kmax + 2]
    assert len(src) >= lens[-1]
    return [("softmask_all[:%d]" % n, src[:n]) for n in lens]


# paths of the replays of the reference's call-history caches (snipmemo.h: SnipCount; assmemo.h: AssCount), in the order of the counters
SNIP_COUNTERS = ("windows", "merged", "merged_3steps", "clamp_start", "clamp_end", "max_blocks", "empty_block_wins", "pieces_3win",
                 "get_empty", "get_extend", "get_hit", "get_none", "get_part", "add_same", "map_fallback", "col0_req", "below_row0",
                 "mixed_same", "patch_fwd", "patch_rev", "wins_3planes")
ASS_COUNTERS = ("calls", "flushes", "skips", "skipped_sites", "flush_in_skip", "first_longass", "first_utr5internal", "first_utr5term",
                "first_utr3internal", "first_utr3term", "long_foreign", "sites_0changes", "sites_1change", "sites_2changes", "extras",
                "late_calls", "late_flushes", "vit_diffs")
REPLAY_MAXIMA = ("max_blocks",)  # (a maximum, not a count)


def merge_counters(a, b):
    return {k: (max(a.get(k, 0), v) if k in REPLAY_MAXIMA else a.get(k, 0) + v) for k, v in b.items()}


def _replay_out(counters, patches, sites):
    """(n, snip[], ass[], tss), (keys [n][4], te) and recs [m][4] -> ({counter: value}, {piece: {(j, s, eop): te}}, {piece: [(q, key, class)]})"""
    code, snip, ass, tss = counters
    assert code == len(SNIP_COUNTERS) * 100 + len(ASS_COUNTERS), code
    cnt = dict(zip(SNIP_COUNTERS, snip))
    cnt.update(zip(ASS_COUNTERS, ass))
    cnt["tss_changed"] = tss
    terms, hist = {}, {}
    for k, v in zip(*patches):
        d = terms.setdefault(k[0], {})
        assert tuple(k[1:]) not in d, k  # (a candidate is patched once)
        d[tuple(k[1:])] = v
    for r in sites:
        hist.setdefault(r[0], []).append(tuple(r[1:]))
    return cnt, terms, hist


def _replay_fetch(get_counters, get_patches, get_sites):
    snip, ass, tss = (ctypes.c_longlong * 64)(), (ctypes.c_longlong * 64)(), ctypes.c_longlong()
    code = get_counters(snip, ass, ctypes.byref(tss))
    n = get_patches(None, None, ctypes.c_int64(0))
    keys, te = np.zeros((max(n, 1), 4), dtype=np.int32), np.zeros(max(n, 1))
    assert get_patches(keys.ctypes.data_as(ctypes.c_void_p), te.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(n)) == n
    m = get_sites(None, ctypes.c_int64(0))
    recs = np.zeros((max(m, 1), 4), dtype=np.int32)
    assert get_sites(recs.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(m)) == m
    return _replay_out((code, list(snip[:len(SNIP_COUNTERS)]), list(ass[:len(ASS_COUNTERS)]), tss.value),
                       (keys[:n].tolist(), te[:n].tolist()), recs[:m].tolist())


def emu_replay_log(lib=None):
    """what the cache replays of the last emu_decode did: ({counter: value}, {piece: {(j, s, eop): rebuilt term}},
    {piece: [(q, key, class)] in the order of the calls})"""
    E = _emu_of(lib)
    E.emu_replay_patches.restype = E.emu_replay_sites.restype = ctypes.c_int64
    return _replay_fetch(E.emu_replay_counters, E.emu_replay_patches, E.emu_replay_sites)


def batch_replay_log(batch):
    """the same from a decoded batch of the device library (augustus_amd.Batch.replay_hooks)"""
    return _replay_fetch(*batch.replay_hooks())


def _two_class_piece(seed, head=1000, mid=5000, tail=1000):
    """two GC classes under human (measured with the twin): 68 % GC, 36 %, 68 % -- the class steps lie about 1.7 kb from either end"""
    return _gc_dna(head, 0.68, seed) + _gc_dna(mid, 0.36, seed + 1000) + _gc_dna(tail, 0.68, seed + 2000)


def _ag_rich(n, gc, seed, every):
    """random DNA of the given GC content with an AG about every `every` bases: some 2000 acceptor sites in 9 kb"""
    rng = random.Random(seed)
    s = list(_gc_dna(n, gc, seed))
    i = rng.randrange(every)
    while i + 1 < n:
        s[i], s[i + 1] = "A", "G"
        i += rng.randint(every - 2, every + 2)
    return "".join(s)


# The models of the replay tests.  The class steps of a piece lie between GCwinsize / 2 + 1 and len - GCwinsize / 2 (the stairs hold the
# class of the first window up to there and of the last window from there; smoothing only removes steps).  A replay window is clamped at
# the start of its piece for a step below d + 64 and at its end for a step above len - 2 d - 65: with the models' own windows (human
# 3000 with d = 584, all others 10 000 with d <= 950) no window of any piece is clamped.  GCwinsize is an option of the reference:
# at 600 (human) the steps come within 301 bases of either end.
REPLAY_CFGS = {
    "human": ("human", {"softmasking": "0"}),
    "human_w600": ("human", {"softmasking": "0", "GCwinsize": "600"}),
    "nasonia_w1000": ("nasonia", {"UTR": "off", "sample": "0", "softmasking": "0", "GCwinsize": "1000"}),
    "human_utr": ("human", {"UTR": "on", "softmasking": "0"}),
    "human_utr_w600": ("human", {"UTR": "on", "softmasking": "0", "GCwinsize": "600"}),
}
REPLAY_DENSE = ("human_utr", "human_utr_w600")


def replay_batch_pieces(n_multi=13, distinct=None):
    """[(name, sequence)]: n_multi pieces with two GC classes under human (class steps near 1720 and 5245) and a single-class piece of
    2 kb after each: more multi-class pieces than the replay of a batch with a matrix has workers (12), at piece indices above 0.
    distinct: that many different two-class sequences, taken in turn (the oracle decodes a sequence once)"""
    recs = []
    for k in range(n_multi):
        q = k % (distinct or n_multi)
        recs.append(("two%d" % q, _two_class_piece(5 + q)))
        recs.append(("one%d" % k, _gc_dna(2000, 0.40, 700 + k)))
    return recs


def replay_edge_cases():
    """{configuration of REPLAY_CFGS: [(name, sequence, init_kind, term_kind)]}, pieces of at most 12 kb made for the paths of the cache
    replays (snipmemo.h, assmemo.h) that the other fixtures do not reach; tests/test_emu_replay.py shows from the replays' counters that
    they do (found by a search on the CPU, driven by those counters):
    - a class step 474 bases after the piece start, one some 470 before the end (pieces of different lengths: entry 0 of the reference's
      TSS caches lives on between sequences of one length, tests/test_memo_replay.py), both in one piece (one merged window, clamped on either
      side), the last also as an interior cut (init_kind = term_kind = 1): the j = 1 start of a window, predecessors in column 0;
    - nasonia (d = 950, five classes) over a GC gradient: six steps in one window of 862 blocks of 8 bases that reads four planes;
    - the 13 two-class pieces of replay_batch_pieces among single-class ones, as one batch;
    - UTR states: 9 kb with an AG every 4 bases and four or five GC stretches -- the aSSProb memo is emptied 19 (ag5) and 20 (ag4) times, also inside the
      range a requester skips, sites change their value twice, each of the five requester kinds asks first; an AG in the last bases;
      7.2 kb with an AG every 3 bases (238 flushes): a requester comes back to a range it has walked when the memo is full, and
      to sites above the one at which its own walk emptied the memo (a walk that skips either is told apart from the call-by-call
      one by this piece alone)"""
    ends = [("step_start", _gc_dna(400, 0.70, 1) + _gc_dna(3000, 0.34, 2), 0, 0),
            ("step_end", _gc_dna(3100, 0.34, 3) + _gc_dna(400, 0.72, 4), 0, 0),
            ("step_both", _gc_dna(350, 0.72, 5) + _gc_dna(1500, 0.34, 6) + _gc_dna(350, 0.72, 7), 0, 0),
            ("step_both_cut", _gc_dna(350, 0.72, 5) + _gc_dna(1500, 0.34, 6) + _gc_dna(350, 0.72, 7), 1, 1)]
    grad = "".join(_gc_dna(700, g, 10 + i) for i, g in enumerate((0.25, 0.32, 0.38, 0.44, 0.5, 0.56, 0.62, 0.56, 0.44, 0.32)))
    ag5 = "".join(_ag_rich(1800, g, i, 4) for i, g in enumerate((0.34, 0.72, 0.34, 0.72, 0.34)))
    ag4 = "".join(_ag_rich(2300, g, 10 + i, 4) for i, g in enumerate((0.70, 0.34, 0.70, 0.34)))
    ag3 = "".join(_ag_rich(1200, g, 779858 + i, 3) for i, g in enumerate((0.34, 0.72, 0.34, 0.72, 0.34, 0.72)))
    two = [(n, s, 0, 0) for n, s in replay_batch_pieces(2)]
    return {
        "human": two,
        "human_w600": ends,
        "nasonia_w1000": [("gradient", _gc_dna(1500, 0.25, 9) + grad + _gc_dna(1500, 0.3, 8), 0, 0)],
        "human_utr": two[:2],
        "human_utr_w600": ends + [("ag5", ag5, 0, 0), ("ag4", ag4, 0, 0), ("ag_end", ag4[:2300] + ag5[:1800] + "CAGAG", 0, 0), ("ag3", ag3, 0, 0)],
    }


_replay_models, _replay_twins = {}, {}


def replay_model(cfg, **more):
    import augustus_amd as ax
    key = (cfg, tuple(sorted(more.items())))
    if key not in _replay_models:
        species, opts = REPLAY_CFGS[cfg]
        _replay_models[key] = ax.Model(config_path(), species, **{**opts, **more})
    return _replay_models[key]


def replay_twin(cfg, case):
    """(twin_decode's tuple with cells, {key: term}, site log, flushes) of one (name, sequence, init_kind, term_kind) under a
    configuration of REPLAY_CFGS, with the twin's caches on; computed once per sequence"""
    name, seq, ik, tk = case
    key = (cfg, seq, ik, tk)
    if key not in _replay_twins:
        m = replay_model(cfg)
        _replay_twins[key] = twin_cache_log(m.tables_ptr, seq, m.n_states, cells=True, init_kind=ik, term_kind=tk)
    return _replay_twins[key]


def assert_terms_equal(got, want, what):
    """{key: term} against {key: term}: both directions, bit for bit"""
    missing = sorted(set(want) - set(got))
    extra = sorted(set(got) - set(want))
    assert not missing and not extra, (what, "not patched", missing[:5], len(missing), "patched, not in the twin's log", extra[:5], len(extra))
    wrong = [(k, got[k], want[k]) for k in want if got[k] != want[k]]
    assert not wrong, (what, wrong[:5], len(wrong))


# ---------------------------------------------------------------------------------------------------
# the near-tie counter against the twin's definition (tests/test_emu_ties.py, tests/test_gpu_ties.py; DESIGN.md 6 "near-ties")
# ---------------------------------------------------------------------------------------------------
TIES_CFGS = {**GOLDEN_CFGS, **GENEMODEL_CFGS, "caenorhabditis": ("caenorhabditis", {"UTR": "off", "sample": "0", "softmasking": "0"}),
             "maize": ("maize", {"UTR": "off", "sample": "0", "softmasking": "0"})}
# (configuration, AUGX_BLK or None: the model's own block size)
TIES_TRELLIS = [("human", None), ("caenorhabditis", None), ("human", "2")]
TIES_DENSE = [("human_utr", "4"), ("human_utr", "2"), ("fly_utr", "4"), ("human_atleastone", "8"), ("maize", "8")]
TIES_PRODUCT_EPS = 2e-7  # dp.h: AUGX_NEAR_TIE
# The large threshold of each configuration, chosen from the twin's margins (DESIGN.md 6 has the flagged share of every record): with it
# every record named in TIES_ON_PATH has between 1 % and 50 % of the chain cells of its path flagged, which the tests assert
TIES_EPS = {"human": 20.0, "caenorhabditis": 20.0, "human_utr": 20.0, "fly_utr": 20.0, "human_atleastone": 20.0, "maize": 20.0}
# a second large threshold for the UTR site-list branch of the dense back-trace: at 20.0 the candidate BEHIND a runner-up that shares the
# winner's predecessor end lies within the threshold as well, so the count cannot tell whether pass 1 excluded the winner by its end
# alone; at 12.0 it does on withN (1 % to 50 % of the chain cells of its path are flagged there too, asserted)
TIES_EPS_SHARED_END = 12.0
_ties_twin = {}


def ties_family(cfg):
    """0: the configuration is decoded by the trellis kernels, 1: by the dense kernels"""
    return 1 if cfg in [c for c, _ in TIES_DENSE] else 0


def ties_twin(m, cfg, seq, init_kind=0, term_kind=0, tag=None):
    """TwinTies of one record under configuration cfg, computed once per process (the twin knows neither AUGX_BLK nor the threshold).
    Follows AUGX_EXACT_MULTICLASS like twin_decode.  tag: names the model m when it is not the one of TIES_CFGS[cfg]"""
    key = (tag or cfg, seq, init_kind, term_kind, os.environ.get("AUGX_EXACT_MULTICLASS", "1") != "0")
    if key not in _ties_twin:
        _ties_twin[key] = TwinTies(m.tables_ptr, seq, m.n_states, ties_family(cfg), init_kind, term_kind)
    return _ties_twin[key]


def ties_share(T, eps):
    """share of the chain cells on the twin's path that are flagged at threshold eps"""
    on = [it for it in T.items if it[2] < 2]
    return sum(1 for it in on if it[3] < eps) / max(1, len(on))


def ties_first_diff(flags, T, eps):
    """None when the flags a decode left ([n, S] as chain_flags_of) equal the twin's for every chain cell of every base >= 1 -- live where
    the twin's cell is live, flagged where the twin's margin is below eps --, else a text that names the first cell that differs"""
    want = T.flags(eps)
    want[0, :] = -1
    # (-2: the dense kernels' mark of a piece of N only, written for the synch state whether or not its cell is live: no decision, no
    # flag.  Allowed in a piece without a nucleotide only: anywhere else it is a difference)
    if T.all_n:
        flags = np.where((flags == -2) & (want != 1), want, flags)
    bad = np.argwhere(flags != want)
    if len(bad) == 0:
        return None
    j, s = (int(x) for x in bad[0])
    return "%d chain cells differ, first at base %d state %d: %d against the twin's %d (margin %r)" % (len(bad), j, s, flags[j, s], want[j, s], T.margin[j, s])


K_RSINGLE, K_RTERMINAL, K_UTR5SINGLE = 5, 8, 19  # include/augx.h: AUGX_K_RSINGLE, AUGX_K_RTERMINAL, AUGX_K_UTR5SINGLE (the first UTR kind)


def ties_conditions(T, eps, R, chain_states, kinds=None, dense=False):
    """the shapes the inputs of the near-tie tests are there for, as the TWIN's path and margins show them at threshold eps (R: the bases of
    a chain run that one round of loads of the back-trace covers).  The in-round distance of a cell of a chain run is (top of the run -
    base) mod R, as the back-trace walks the run down from its top; in the trellis family the pair of bases at distances 128 j + 2 l and
    + 1 is load j of lane l.  Returns a set of names:
      flag_d0 / _d1 / _dR-2 / _dR-1 / _next0: a flagged cell at that in-round distance (next0: distance 0 of the second round) in a run
        longer than 2 R; noflag_...: an unflagged cell there beside a flagged cell of the same run;
      entry_flag_d0 / entry_flag_dR-1 / entry_noflag_d0 / entry_noflag_dR-1: a run entered from another state inside the piece whose entry
        cell is at that in-round distance, flagged / not; entry_flag, entry_noflag: at any distance;
      run_to_base1: a run that reaches base 1; flag_base1, flag_last_base: a flagged cell on the path at base 1 / the last base of the piece;
      lane0, lane63: a flagged cell of the path in lane 0 / 63 of a load (dense=True: of a chunk of the dense back-trace's count loop, which
        goes up from the entry cell; flag_tail_chunk: a flagged cell in its last, partly filled chunk); slot<c>: a flagged cell of the path in chain slot c;
      cells_slot<c>: a flagged cell anywhere in the matrix in chain slot c; var<state>: a counted variable-length element of that state;
      var_tie: a variable-length element of the path with an exact tie (margin 0: not counted);
      with kinds (the AUGX_K_* kind of every state), per branch of the back-trace that takes the arg-max of such an element again -- rec: the
      candidate records of kCand (coding exons, lessD), utr: the UTR site list (UTR exon kinds; AUGX_K_UTR5SINGLE = 19 and above) --
      var_chunks_<branch>: a counted element whose cell has more than 64 live candidates (predecessor end, ancestor): more than one chunk
      of a wavefront in both passes; var_same_<branch>: a counted element whose runner-up shares the winner's predecessor end and differs
      in the ancestor (pass 1 must exclude the winner by both); var_shared_end_<branch>: an element of the path, counted or not, some two
      live candidates of whose cell share a predecessor end"""
    conds = set()
    on = {(b, s): mk for b, s, rule, mk, mf in T.items if rule < 2}
    tags = {0: "d0", 1: "d1", R - 2: "dR-2", R - 1: "dR-1"}
    for b, e, s, _ in T.path:
        if s not in chain_states:
            continue
        fl = [on[(q, s)] < eps for q in range(b, e + 1)]
        slot = chain_states.index(s)
        for i, f in enumerate(fl):
            q, d = b + i, (e - b - i) % R
            near = (i > 0 and fl[i - 1]) or (i + 1 < len(fl) and fl[i + 1])
            if e - b + 1 > 2 * R:
                for tag in ([tags[d]] if d in tags else []) + (["next0"] if e - q == R else []):
                    if f:
                        conds.add("flag_" + tag)
                    elif near:
                        conds.add("noflag_" + tag)
            if f:
                conds.add("slot%d" % slot)
                # (trellis back-trace: the cells are counted from the loads of the walk; dense back-trace, dense.h:1434-1440: counted in a
                # loop of its own that goes up from the entry cell of the run -- or base 1 -- 64 cells at a time, lane = cell - entry mod 64)
                lane = (i % 64) if dense else (d % 128) // 2
                if lane in (0, 63):
                    conds.add("lane%d" % lane)
                if dense and (e - b + 1) % 64 != 0 and i >= (e - b + 1) // 64 * 64:
                    conds.add("flag_tail_chunk")  # (the last chunk of the count loop, some of whose lanes lie above the top of the run)
        if b > 1:
            d = (e - b) % R
            conds.add("entry_flag" if fl[0] else "entry_noflag")
            if d in (0, R - 1):
                conds.add(("entry_flag_" if fl[0] else "entry_noflag_") + tags[d])
        else:
            conds.add("run_to_base1")
            if fl[0]:
                conds.add("flag_base1")
        if e == T.n - 1 and fl[-1]:
            conds.add("flag_last_base")
    f = T.flags(eps)
    for c, s in enumerate(chain_states):
        if (f[1:, s] == 1).any():
            conds.add("cells_slot%d" % c)
    for b, s, rule, mk, mf in T.items:
        if rule == 2 and 0 < mk < eps:
            conds.add("var%d" % s)
        if rule == 2 and mk == 0:
            conds.add("var_tie")
        if rule == 2 and 0 < mk < eps and kinds is not None:
            # (the branch of the back-trace that takes the arg-max again: the UTR site list, or the candidate records of kCand)
            br = "utr" if kinds[s] >= K_UTR5SINGLE else "rec"
            if T.cands[(b, s)][0] > 64:
                conds.add("var_chunks_" + br)
            if T.cands[(b, s)][1]:
                conds.add("var_same_" + br)
        if rule == 2 and kinds is not None and T.cands[(b, s)][2]:
            conds.add("var_shared_end_" + ("utr" if kinds[s] >= K_UTR5SINGLE else "rec"))
    return conds


# records the on-path assertions rest on: with TIES_EPS between 1 % and 50 % of the chain cells of the twin's path are flagged
TIES_ON_PATH = {0: ("rand60k", "withN", "multigc_levels", "HS04636", "softmask_all", "multigc_two", "gt_cag", "orf12k", "multi_far", "gcsteps7_0", "gcsteps7_1"),
                1: ("HS04636", "withN", "taa_after_gene", "aataaa_after_gene", "gene_N_runs", "twoclass_gene", "cut_11_1")}
# prefixes found by a search over the twin's list (a chain run whose top is the end of the piece: the length of the prefix sets the
# in-round distance of its cells): (golden record, length) -> the shape it is there for at TIES_EPS (ties_conditions)
TIES_FOUND = {"human": (("HS04636", 2745), ("HS04636", 8951), ("withN", 8125), ("withN", 10173)),   # entry_flag_d0, entry_flag_dR-1, noflag_next0, flag_next0
              "caenorhabditis": (("HS04636", 6904), ("HS04636", 8951), ("multigc_levels", 13652), ("rand60k", 7301)),  # the same four
              "human_utr": (("HS04636", 1564), ("HS04636", 9113)),                                # entry_flag_d0, entry_flag_dR-1
              "fly_utr": (("HS04636", 8850), ("HS04636", 9105), ("HS04636", 9367)), "human_atleastone": (("HS04636", 6904), ("HS04636", 7159)),
              "maize": (("HS04636", 1164), ("HS04636", 1419))}
# the same search for runs whose entry cell is NOT flagged at TIES_EPS (nearly every entry cell is): an edge case that ends in an intergenic
# run with such an entry, a tail of random DNA behind it, cut to the length that puts the entry at in-round distance 0 / R - 1:
# (edge case, seed of the tail, lengths)
TIES_TAILS = {"human": ("orf12k", 4, (15136, 15137)), "caenorhabditis": ("orf12k", 4, (13007,)), "human_utr": ("cag_many", 4, (13520, 13775)),
              "fly_utr": ("cag_many", 5, (13868, 14123)), "human_atleastone": ("orf12k", 4, (13089, 13344)), "maize": ("orf12k", 4, (13007, 13262))}


# windows of 20 kb of the real DNA the soaks draw from (tests/soak_cli.py: real_dna; window w = bases 20 000 w .. 20 000 (w + 1)), found by
# the same search: paths with a flagged cell in chain slot 3 (the geometric intron state of frame 2) and with counted elements of the
# kinds the edge cases do not count
# (negative: window -w in upper case -- a third of this DNA is soft-masked, and the masked bases are hints against exons)
TIES_REAL_WINDOWS = {"maize": (7, 10, 31), "fly_utr": (1, 3, 4, 11, 28, 29, 38, -3, -4), "human_atleastone": (1, 3), "human_utr": (1, 3, 4, -1, -4)}
_real_dna = None


def ties_real_windows(cfg):
    global _real_dna
    if cfg not in TIES_REAL_WINDOWS:
        return []
    if _real_dna is None:
        import soak_cli
        _real_dna = soak_cli.real_dna()[1]
    win = lambda w: _real_dna[abs(w) * 20000:(abs(w) + 1) * 20000]
    return [("real[%d]%s" % (abs(w), " upper" if w < 0 else ""), win(w).upper() if w < 0 else win(w)) for w in TIES_REAL_WINDOWS[cfg]]


def ties_tail_records(cfg):
    base, seed, lens = TIES_TAILS[cfg]
    R = emu_trellis_windows()["BT_ROUND_DENSE" if ties_family(cfg) else "BT_ROUND"]
    tr = dict(trellis_edge_cases())
    head = tr[base][:-1000] if base == "orf12k" else tr[base][:-2000]  # (the edge case without its own tail)
    seq = head + random_dna((2200 if base == "orf12k" else 2000) + 3 * R, seed)
    recs = [("%s_tail%d[:%d]" % (base, seed, n), seq[:n]) for n in lens]
    if cfg == "caenorhabditis":  # (its second length came from another tail)
        recs.append(("orf12k_tail9[:15054]", (head + random_dna(2200 + 3 * R, 9))[:15054]))
    return recs


def ties_n_jump_record():
    """5 kb of the golden record withN on either side of a run of 3600 N, which the trellis jumps over (a run of 3000 it does not): the
    twin's path is one intergenic run through it"""
    w = dict(golden_inputs())["withN"]
    return ("N_jump", w[15000:20000] + "N" * 3600 + w[23000:28000])


def ties_records(cfg):
    """[(name, sequence)] of the near-tie tests of one configuration: the golden records, the edge cases of the family's kernels, two
    records whose GC content steps, pieces of a few bases, one intergenic run (prefixes of softmask_all) and runs of N of the lengths
    around one, two and three rounds of the back-trace (tests/test_gpu_backtrace.py has every length 1..300 and 256 k + d up to 7 936
    because it does not know the round; here R is exported and the lengths are the edges of the first three rounds), and the prefixes
    and tails found by search (TIES_FOUND, TIES_TAILS)"""
    fam = ties_family(cfg)
    by = dict(golden_inputs())
    R = emu_trellis_windows()["BT_ROUND_DENSE" if fam else "BT_ROUND"]
    if fam:
        recs = [(k, by[k]) for k in ("HS04636", "withN", "short7", "short100", "revcomp", "rand20k_b", "HS08198")]
        recs += dense_edge_cases()
    else:
        recs = [(k, by[k]) for k in ("rand60k", "withN", "multigc_levels", "HS04636", "softmask_all", "multigc_two", "short7", "short100")]
        recs += [(k, by[k]) for k in ("revcomp", "rand20k_b", "HS08198")]
        recs += trellis_edge_cases() + gc_step_records(2, 7)
        recs.append(("cag_dense", "ACGT" * 500 + "CAG" * 2500 + "ACGT" * 500))  # (dense_edge_cases: cells with more than 64 live candidates)
        recs.append(ties_n_jump_record())
    lens = sorted({1, 2, 3, 4} | {k * R + d for k in (1, 2, 3) for d in (-1, 0, 1, 2)})
    recs += [("softmask_all[:%d]" % n, by["softmask_all"][:n]) for n in lens if n <= len(by["softmask_all"])]
    recs += [("N*%d" % n, "N" * n) for n in lens if n <= 2 * R + 2]
    recs += [("%s[:%d]" % (k, n), by[k][:n]) for k, n in TIES_FOUND.get(cfg, ())]
    recs += ties_tail_records(cfg) + ties_real_windows(cfg)
    assert len(set(n for n, _ in recs)) == len(recs)
    return recs


TIES_CORE = {"flag_d0", "flag_d1", "flag_dR-2", "flag_dR-1", "noflag_d0", "noflag_d1", "noflag_dR-2", "noflag_dR-1", "lane0", "lane63",
             "run_to_base1", "flag_last_base", "entry_flag", "flag_next0", "noflag_next0", "entry_flag_d0", "entry_flag_dR-1", "entry_noflag",
             "entry_noflag_d0", "entry_noflag_dR-1"}
_DENSE_VAR = {"flag_tail_chunk", "var_tie", "var_chunks_rec", "var_same_rec", "var_chunks_utr", "var_same_utr"}
# what the records of a configuration show at TIES_EPS on top of TIES_CORE (ties_conditions; asserted from the twin's output).  Not there:
# a flagged cell at base 1 under the model with two intergenic states (its first intergenic state has one way in); UTR branches under the
# models without UTR states; under the 47-state models no two live candidates of a variable-length cell share a predecessor end (one
# feasible ancestor per end: lessD has one ancestor, the reading frame picks the one of an exon), so var_same_rec cannot exist there --
# the tests assert that var_shared_end_rec is absent -- and no DNA with an exactly tied element was found (var_tie; DESIGN.md 6 lists the
# searches): tests/test_emu_ties.py reaches that tie through the model (BumpedTables)
TIES_SHAPES = {
    "human": {"flag_base1", "var_chunks_rec"}, "caenorhabditis": {"flag_base1", "var_chunks_rec"},
    "human_utr": {"flag_base1"} | _DENSE_VAR, "fly_utr": {"flag_base1"} | _DENSE_VAR,
    "human_atleastone": {"flag_tail_chunk", "var_same_rec"}, "maize": {"flag_base1", "flag_tail_chunk", "var_chunks_rec"},
}
TIES_ONE_ANCESTOR_PER_END = ("human", "caenorhabditis", "maize")
# What cannot be there.  Chain slot 0 under the model with two intergenic states: its first intergenic state has one way in, so its cells
# have no runner-up and no flag.  Reverse single (AUGX_K_RSINGLE, 5) and reverse terminal (AUGX_K_RTERMINAL, 8) exons under the 47-state
# models: one predecessor end, the reading frame's, and one ancestor -- one candidate, no runner-up (under the UTR models and under two
# intergenic states they have more ancestors and ARE counted).  What is merely not there: the internal UTR exons of human --UTR=on (kinds
# 23, 29, 35, 41: a UTR with two introns) -- none of the 50 windows of the real DNA, raw or in upper case, has one on its path under human;
# fly --UTR=on counts 23, 35 and 41
TIES_NO_SLOT = {"human_atleastone": {0}}
TIES_KINDS_UNCOUNTED = {"human": {5, 8}, "caenorhabditis": {5, 8}, "maize": {5, 8}, "human_utr": {23, 29, 35, 41}, "fly_utr": set(), "human_atleastone": set()}


def emu_seg_stops(lib=None):
    """[(index in the piece, first tile, end tile, seg_stop, seg_stop2)] of the segments of the emulator's last decode by the trellis kernels
    (tiles of 64 bases; the stops as Batch.plan gives them on the device)"""
    out = np.zeros((64, 5), dtype=np.int32)
    n = _emu_of(lib).emu_seg_stops(out.ctypes.data_as(ctypes.c_void_p), 64)
    rows, k, prev = [], 0, None
    for piece, t0, t1, stop, stop2 in out[:n].tolist():
        k = k + 1 if piece == prev else 0
        prev = piece
        rows.append((k, t0, t1, stop, stop2))
    return rows


def ties_assert_rewritten_tiles(T, eps, segs, nocheck):
    """the twin T of ONE piece decoded in segments has flagged chain cells in the tiles that a fix-up rewrote, in those a continuation
    rewrote and -- nocheck: an unreachable check length -- in those left to the last pass.  segs: [(index in the piece, first tile, end
    tile, seg_stop, seg_stop2)].  With an unreachable check length all four fix-ups give up; three are continued by the rounds of pass 3
    and the fourth, the last segment's, is left to the last pass (tests/test_emu_trellis.py shows that from the emulator's counters; the
    plan records where either stopped in the same field)"""
    f = (T.flags(eps) == 1).any(axis=1)
    fixed = continued = last = 0
    for k, t0, t1, stop, stop2 in segs:
        if k == 0:
            continue
        end = stop if stop >= t0 - 1 else -2 - stop  # (the last tile the fix-up rewrote, converged or not)
        fixed += int(f[64 * t0:64 * (end + 1)].sum())
        if stop <= -2 and stop2 >= 0:
            continued += int(f[64 * (end + 1):64 * (stop2 + 1)].sum())
            if nocheck and k == len(segs) - 1:
                last += int(f[64 * (end + 1):64 * (stop2 + 1)].sum())
    assert sum(1 for k, _, _, stop, _ in segs if k > 0 and stop <= -2) == (len(segs) - 1 if nocheck else 1), segs
    assert fixed > 0 and continued > 0 and (last > 0 or not nocheck), (fixed, continued, last)
