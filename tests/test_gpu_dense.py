"""The inputs made for the rare data paths of the dense kernels (helpers.dense_edge_cases, helpers.dense_backtrace_prefixes;
tests/test_emu_dense.py shows from the emulator's counters that they take those paths) on the GPU, where the emulator, which is
sequential, cannot stand in: units of one descriptor handed to several wavefronts, LDS atomics of several units into one cell, the
ring against HBM at distances 63 and 64 with a global barrier only every 32 bases, the next block's descriptors staged while seven
wavefronts read this block's.
- kUtrDesc, kDense<BLK, 0, false>, kDense<BLK, 0, true> (near ties counted) and kDenseBacktrace under the 71-state model at block sizes
  4 and 2 (human) and 4 (fly), the 48-state model with two intergenic states and maize at 8: one batch in the given order and one
  reversed, each decoded twice: status, score, path and every cell equal the oracle twin's;
- the same with a descriptor buffer that is too small at first (AUGX_UD_CAP=16): kUtrDesc runs twice;
- kDense<BLK, 1> against every forward variable of the live reference, cold and heated, and bit-equal run after run;
- the chain runs of the back-trace around its steps of 256 bases;
- all of the first item with the dense kernels built for 8 descriptors of a block in LDS (augustus_amd/libaugx_smallwin.so, loaded by a
  fresh child process through AUGX_LIB), where most descriptors of a block are read from HBM."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import augustus_amd as ax
from helpers import *

DENSE_GPU = [("human_utr", "4"), ("human_utr", "2"), ("fly_utr", "4"), ("human_atleastone", "8"), ("maize", "8")]
CFGS = {**GOLDEN_CFGS, **GENEMODEL_CFGS, "maize": ("maize", {"UTR": "off", "sample": "0", "softmasking": "0"})}
_want = {}


@pytest.fixture(autouse=True)
def _one_class_per_end_base(monkeypatch):
    """exact mode off, as in test_gpu_parity.py: decoders are created with the first pass on its own, and the twin's restatement of the
    snippet cache is off with it"""
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")


def _twin(m, cfg, seq, cells=True):
    """the twin's (status, score, path, cells) of one record under configuration cfg, computed once (the twin does not know AUGX_BLK,
    the near-tie build or the order of the batch).  The caller has AUGX_EXACT_MULTICLASS=0 set: twin_decode follows it"""
    key = (cfg, seq)
    if key not in _want:
        assert os.environ.get("AUGX_EXACT_MULTICLASS") == "0"
        rc, lnv, path, V, _ = twin_decode(m.tables_ptr, seq, m.n_states, cells=cells)
        # (two intergenic states: a record without room for a gene has no feasible path; its cells are compared all the same)
        assert rc == 0 or (cfg == "human_atleastone" and rc == ax.AUGX_E_NOPATH)
        _want[key] = (rc, lnv, path, V)
    return _want[key]


def _check_batch(m, cfg, b, seqs, cells=True):
    res = b.paths()
    assert len(res) == len(seqs)
    for i, (seq, r) in enumerate(zip(seqs, res)):
        rc, lnv, path, V = _twin(m, cfg, seq, cells)
        assert r.status == rc, (i, r.status, rc)
        if rc == 0:
            assert r.ln_viterbi == lnv and r.states == path, i
        if cells:
            assert np.array_equal(b.cells(i), V), i


def _model(cfg, blk):
    os.environ["AUGX_BLK"] = blk
    species, opts = CFGS[cfg]
    return ax.Model(config_path(), species, **opts)


def _decode_and_check(m, cfg, seqs, ties):
    d = ax.Decoder(m, 0)
    d.count_near_ties(ties)  # (True: batches created from now on run kDense<., 0, true>)
    for order in (seqs, seqs[::-1]):
        b = ax.Batch(d, order)
        b.decode()
        _check_batch(m, cfg, b, order)
        b.decode()  # (the same batch again: the buffers hold what the first decode left)
        _check_batch(m, cfg, b, order)
        b.close()
    d.close()


def check_library(cfgs, ties):
    """the body of the tests below, for the library this process has loaded (the caller sets AUGX_EXACT_MULTICLASS=0)"""
    saved = os.environ.get("AUGX_BLK")
    os.environ["AUGX_DEBUG_CELLS"] = "1"
    seqs = [s for _, s in dense_edge_cases()]
    try:
        for cfg, blk in cfgs:
            m = _model(cfg, blk)
            for t in ties:
                _decode_and_check(m, cfg, seqs, t)
    finally:
        os.environ.pop("AUGX_DEBUG_CELLS", None)
        os.environ.pop("AUGX_BLK", None)
        if saved is not None:
            os.environ["AUGX_BLK"] = saved


@pytest.mark.parametrize("ties", [False, True], ids=["plain", "near_ties"])
@pytest.mark.parametrize("cfg,blk", DENSE_GPU)
def test_gpu_dense_edge_cases_bit_identical_to_oracle(monkeypatch, cfg, blk, ties):
    monkeypatch.setenv("AUGX_BLK", blk)  # (restored after the test; check_library sets it itself)
    monkeypatch.setenv("AUGX_DEBUG_CELLS", "1")
    check_library([(cfg, blk)], [ties])


@pytest.mark.parametrize("cfg,blk", [c for c in DENSE_GPU if "utr" in c[0]])
def test_gpu_dense_edge_cases_grown_descriptor_buffer(monkeypatch, cfg, blk):
    """a first estimate of 16 descriptors for a batch that has tens of thousands: kUtrDesc reports the count, the buffer grows, the
    kernel runs again -- now on blocks with many descriptors"""
    monkeypatch.setenv("AUGX_UD_CAP", "16")
    monkeypatch.setenv("AUGX_BLK", blk)
    monkeypatch.setenv("AUGX_DEBUG_CELLS", "1")
    check_library([(cfg, blk)], [False])


def test_gpu_dense_small_descriptor_staging():
    """the dense kernels built with AUGX_UDCAP=8 (Makefile: libaugx_smallwin.so): the same bit equality under every configuration.  A
    fresh process: the library is chosen when augustus_amd is imported"""
    assert os.path.exists(SMALLWIN_LIB), "augustus_amd/libaugx_smallwin.so is missing: `make product` builds it"
    env = dict(os.environ, AUGX_LIB=SMALLWIN_LIB, AUGX_EXACT_MULTICLASS="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    for k in ("AUGX_BLK", "AUGX_UD_CAP"):
        env.pop(k, None)
    code = ("import augustus_amd as ax, test_gpu_dense as t; assert ax.LIB_PATH.endswith('libaugx_smallwin.so'); "
            "t.check_library(t.DENSE_GPU, [False]); t.check_library(t.DENSE_GPU[:1], [True]); print('small staging ok')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=os.path.join(ROOT, "tests"), timeout=600)
    assert r.returncode == 0 and "small staging ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("ties", [False, True], ids=["plain", "near_ties"])
@pytest.mark.parametrize("cfg,kmax", [("fly_utr", 31), ("maize", 31), ("human_utr", 27)])
def test_gpu_dense_backtrace_runs_at_the_step_edges(monkeypatch, cfg, kmax, ties):
    """prefixes of the golden record softmask_all of n = 1..300 and n = 256 k + d bases: ONE intergenic run of n - 1 bases each (asserted
    from the twin's path, so that a record that loses this shape cannot hide a failure), one batch decoded twice"""
    monkeypatch.delenv("AUGX_BLK", raising=False)
    species, opts = CFGS[cfg]
    m = ax.Model(config_path(), species, **opts)
    recs = dense_backtrace_prefixes(kmax)
    for name, seq in recs:
        rc, lnv, path, _ = _twin(m, cfg, seq, cells=False)
        assert rc == 0 and [p[:2] for p in path] == ([(1, len(seq) - 1)] if len(seq) > 1 else []), name
    seqs = [s for _, s in recs]
    d = ax.Decoder(m, 0)
    d.count_near_ties(ties)
    b = ax.Batch(d, seqs)
    for turn in range(2):
        b.decode()
        _check_batch(m, cfg, b, seqs, cells=False)
    b.close()
    d.close()


@needs_ref
@pytest.mark.parametrize("cfg,t", [("human_utr_nosm", 0), ("fly_utr", 0), ("human_utr_nosm", 3), ("fly_utr", 3)])
def test_gpu_dense_forward_edge_cases_match_reference(tmp_path, monkeypatch, cfg, t):
    """every forward variable of the records of dense_edge_cases on the device against the live reference: identical live cells,
    |ln F - reference| <= 1e-9 |reference| + 5e-9, cold and at --temperature=3; and a second forward run of the
    same batch gives the same bits -- the fixed-point sum of a cell does not depend on the order the atomics of its units arrive in"""
    monkeypatch.delenv("AUGX_EXACT_MULTICLASS")  # (the replay of the reference's caches: two records have two classes under human)
    monkeypatch.delenv("AUGX_BLK", raising=False)
    species, opts = CFGS[cfg]
    recs = dense_edge_cases()
    fa = str(tmp_path / "f.fa")
    write_fasta(fa, recs)
    extra = ["--%s=%s" % kv for kv in opts.items() if kv[0] != "sample"] + (["--temperature=%d" % t] if t else [])
    Fref = ref_forward(fa, species, extra)
    assert len(Fref) == len(recs)
    m = ax.Model(config_path(), species, **{**opts, "sample": "100", "temperature": str(t)})
    d = ax.Decoder(m, 0)
    b = ax.Batch(d, [s for _, s in recs])
    b.decode()
    b.forward()
    first = [b.forward_cells(i) for i in range(len(recs))]
    b.forward()
    worst = 0.0
    for i, ((name, seq), fr, r) in enumerate(zip(recs, Fref, b.paths())):
        F, lnp = b.forward_cells(i)
        assert np.array_equal(F.view(np.uint64), first[i][0].view(np.uint64)) and lnp == first[i][1], name
        assert np.array_equal(np.isfinite(F), np.isfinite(fr)), name
        both = np.isfinite(F)
        if not both.any():
            continue
        diff = np.abs(F[both] - fr[both])
        bar = 1e-9 * np.abs(fr[both]) + 5e-9
        worst = max(worst, float(np.max(diff / bar)))
        assert np.all(diff <= bar), name
        if t == 0 and r.status == 0:  # (cold: the sum over all paths holds the best one)
            assert lnp >= r.ln_viterbi, name
    print("device dense forward %s t=%d: largest |ln F - reference| = %.3g of the bound 1e-9 |reference| + 5e-9" % (cfg, t, worst))
    b.close()
    d.close()
